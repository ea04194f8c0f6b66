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
 *
 * With CMP_GPU_OPT_IMAGE_RAGGED and a context whose frames are independent
 * the table is cut into pieces instead (cmp_image_piece_next): refused frames
 * and large runs of equal frames go the same way as above, every other frame
 * joins a ragged piece, which is one ingest, one encode launch per pass
 * (enc_ragged.hip), one scan and one emit.  With
 * CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM a checksum-enabled context takes the
 * pieces too: one ragged XXH32 per piece (checksum.hip) ahead of its encode
 * launches, which append the four bytes.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cmp.h"
#include "cmp_errors.h"
#include "cmp_gpu.h"
#include "airs_dev.h"
#include "cmp_engine.h"
#include "cmp_image_plan.h"
#include "cmp_pass.h"

#define BATCH_FLAGS (CMP_GPU_AUTO_RICE | CMP_GPU_HOST_STEPPED | CMP_GPU_STEPWISE)

static uint32_t up16(uint32_t v)
{
	return (v + 15u) & ~15u;
}

static uint32_t up8(uint32_t v)
{
	return (v + 7u) & ~7u;
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

/* one call's state */
struct image_job {
	struct cmp_gpu_engine *engine;
	struct airs_dev_engine *dev;
	struct cmp_context *ctx;
	const struct cmp_gpu_encode_image *img;
	uint32_t sample_bytes, first_run;
	uint32_t *bound;   /* host [num_frames], 0 for a refused frame: ragged calls only (else NULL) */
	uint64_t keep;     /* the keep threshold of a ragged call */
	uint32_t seg;      /* samples per segment of the ragged kernel */
	uint32_t ck;       /* the ragged pieces carry checksums */
	/* engine scratch */
	uint8_t *tables;   /* the sticky word, then d_off, then the ragged tables */
	uint64_t *d_off;   /* the offsets of the frames in src */
	uint8_t *rag;      /* the tables of one ragged piece (struct rag_layout) */
	uint8_t *rows, *frows;
};

/* The batch path can read the run's samples where they are: native-endian, the
 * first frame aligned to the sample size, the offsets an arithmetic
 * progression whose step is at least the frame and a multiple of the sample
 * size. */
static int run_direct(const struct cmp_gpu_encode_image *img, uint64_t first, uint32_t count, uint32_t sample_bytes,
		      uint64_t *stride)
{
	const uint64_t *o = img->offsets + first;
	const uint32_t fb = img->frame_bytes[first];
	uint32_t j;

	if ((img->flags & CMP_GPU_IMG_SRC_BIG_ENDIAN) || ((uintptr_t)img->src + o[0]) % sample_bytes)
		return 0;
	*stride = fb;
	if (count == 1)
		return 1;
	if (o[1] < o[0] || o[1] - o[0] < fb || (o[1] - o[0]) % sample_bytes)
		return 0;
	*stride = o[1] - o[0];
	for (j = 2; j < count; j++)
		if (o[j] < o[j - 1] || o[j] - o[j - 1] != *stride)
			return 0;
	return 1;
}

/* a frame of a ragged piece is read where it lies: native-endian, at a
 * multiple of the sample size (its neighbours do not matter) */
static int frame_direct(const struct cmp_gpu_encode_image *img, uint64_t f, uint32_t sample_bytes)
{
	return !(img->flags & CMP_GPU_IMG_SRC_BIG_ENDIAN) && ((uintptr_t)img->src + img->offsets[f]) % sample_bytes == 0;
}

/* the next piece of the table: the runs of equal frames, or with the ragged
 * option the pieces of cmp_image_piece_next */
static void next_piece(const struct image_job *J, uint64_t f, struct cmp_image_piece *p)
{
	const struct cmp_gpu_encode_image *img = J->img;

	if (J->bound) {
		cmp_image_piece_next(img->frame_bytes, J->bound, img->num_frames, J->engine->image_chunk, J->keep, 0, f, p);
	} else {
		const uint32_t fb = img->frame_bytes[f];
		struct cmp_image_run r;
		uint32_t bound;
		const uint32_t refused = frame_refusal(fb, J->sample_bytes, &bound);

		cmp_image_run_next(img->frame_bytes, img->num_frames, J->engine->image_chunk, cmp_image_run_row(fb, bound),
				   0, f, &r);
		p->first = f;
		p->count = r.count;
		p->kind = refused ? CMP_IMAGE_PIECE_REFUSED : CMP_IMAGE_PIECE_RUN;
	}
}

/* The device tables of one ragged piece of cnt frames and `blocks` blocks, as
 * byte offsets into one region that a single copy uploads: the descriptors of
 * both passes' launches, then the per-frame arrays.  With ck_blocks != NULL the
 * piece carries checksums: the tables of airs_dev_checksum_ragged (sample
 * address, product offset, product workgroups, sample count) and its output,
 * which the encode launches read. */
struct rag_layout {
	size_t desc, dst_off, ids, row_off, ck_src, ck_off, ck_blocks, caps, row_len, ck_n, ck_out, seqs, total;
};

_Static_assert(sizeof(struct cmp_image_ck_block) == sizeof(struct airs_ragged_ck_block), "one table for both");

static void rag_layout(uint32_t cnt, uint64_t blocks, const uint64_t *ck_blocks, struct rag_layout *L)
{
	size_t at = 0;

	L->desc = at;
	at += (size_t)blocks * sizeof(struct airs_ragged_desc);
	L->dst_off = at;
	at += (size_t)cnt * 8u;
	L->ids = at;
	at += (size_t)cnt * 8u;
	L->row_off = at;
	at += (size_t)cnt * 8u;
	L->ck_src = at;
	at += ck_blocks ? (size_t)cnt * 8u : 0u;
	L->ck_off = at;
	at += ck_blocks ? (size_t)cnt * 8u : 0u;
	L->ck_blocks = at;
	at += ck_blocks ? (size_t)*ck_blocks * sizeof(struct cmp_image_ck_block) : 0u;
	L->caps = at;
	at += (size_t)cnt * 4u;
	L->row_len = at;
	at += (size_t)cnt * 4u;
	L->ck_n = at;
	at += ck_blocks ? (size_t)cnt * 4u : 0u;
	L->ck_out = at;
	at += ck_blocks ? (size_t)cnt * 4u : 0u;
	L->seqs = at;
	at += cnt;
	L->total = (at + 31u) & ~(size_t)31u;
}

static uint32_t frame_segs(const struct image_job *J, uint64_t f)
{
	const uint32_t n = J->img->frame_bytes[f] / J->sample_bytes;

	return (n + J->seg - 1u) / J->seg;
}

/* the scan and the emit of one piece (refused: the scan alone) */
static uint32_t piece_emit(struct image_job *J, uint64_t f, uint32_t count, uint32_t frow_cap, const uint64_t *frow_off,
			   uint32_t refused)
{
	const struct cmp_gpu_encode_image *img = J->img;
	struct airs_encode_image q;
	uint32_t e;

	memset(&q, 0, sizeof(q));
	q.stage = AIRS_ENCIMG_EMIT;
	q.count = count;
	q.frows = J->frows;
	q.frow_bytes = up8(frow_cap);
	q.frow_cap = frow_cap;
	q.frow_off = frow_off;
	q.sizes = img->sizes + f;
	q.out_offsets = img->out_offsets + f;
	q.sticky = (uint32_t *)J->tables;
	q.out = img->out;
	q.out_capacity = img->out_capacity;
	q.first_run = J->first_run;
	q.force = refused;
	e = airs_dev_encode_image(J->dev, &q);
	J->first_run = 0;
	return e;
}

/* one run of equal frames through the batch path */
static uint32_t piece_run(struct image_job *J, uint64_t f, uint32_t count)
{
	const struct cmp_gpu_encode_image *img = J->img;
	const uint32_t fb = img->frame_bytes[f];
	uint32_t bound, e;
	const uint32_t refused = frame_refusal(fb, J->sample_bytes, &bound);

	if (!refused) {
		struct cmp_gpu_batch b;
		uint64_t stride = 0;

		memset(&b, 0, sizeof(b));
		b.type = img->type;
		if (run_direct(img, f, count, J->sample_bytes, &stride)) {
			b.src = (const uint8_t *)img->src + img->offsets[f];
			b.src_stride = stride;
		} else {
			struct airs_encode_image q;

			memset(&q, 0, sizeof(q));
			q.stage = AIRS_ENCIMG_INGEST;
			q.count = count;
			q.src = img->src;
			q.offsets = J->d_off + f;
			q.frame_bytes = fb;
			q.swap = (img->flags & CMP_GPU_IMG_SRC_BIG_ENDIAN) != 0;
			q.rows = J->rows;
			q.row_bytes = up16(fb);
			e = airs_dev_encode_image(J->dev, &q);
			if (e)
				return e;
			b.src = J->rows;
			b.src_stride = q.row_bytes;
		}
		b.src_size = fb;
		b.dst = J->frows;
		b.dst_stride = up8(bound);
		b.dst_capacity = bound;
		b.sizes = img->sizes + f;
		b.flags = img->batch_flags;
		e = cmp_batch_compress(J->engine, J->ctx, 1, count, &b);
		if (e)
			return e;
	}
	return piece_emit(J, f, count, bound, NULL, refused);
}

/* One ragged piece: frames [first, first + cnt), none refused.  The context is
 * replayed over them on the host as the batch path replays its frames
 * (batch_replay, cmp_batch.c): every frame's pass, header sequence number and
 * identifier, the draws in table order, the context's final fields.  The
 * frames of a pass share one launch; their tables go up in one copy from
 * pageable memory, which the runtime has staged when the copy call returns
 * (see the offsets' upload in cmp_gpu_compress_image). */
static uint32_t piece_ragged(struct image_job *J, uint64_t first, uint32_t cnt)
{
	const struct cmp_gpu_encode_image *img = J->img;
	const struct cmp_context snap = *J->ctx;
	const uint32_t sb = J->sample_bytes;
	struct rag_layout L;
	struct pass *pass = NULL;
	struct cmp_image_block *blk = NULL;
	struct airs_ragged_desc *desc;
	uint32_t *segs = NULL, *slot0, *gsegs, *active, *caps, *row_len;
	uint64_t *dst_off, *ids, *row_off, blocks = 0, done = 0, at, id;
	uint8_t *hb = NULL, *seqs;
	uint32_t j, g, e = ERRV(GENERIC), staged = 0, max_len = 0, max_cap = 0, slots = 0;
	uint64_t gfirst[2] = {0, 0}, gblocks[2] = {0, 0};
	uint32_t gframes[2] = {0, 0}, gmember[2] = {0, 0};
	uint64_t ck_blocks = 0, ck_bytes = 0;

	for (j = 0; j < cnt; j++)
		blocks += frame_segs(J, first + j);
	if (J->ck)
		ck_bytes = cmp_image_ck_layout(img->frame_bytes + first, sb, cnt, NULL, NULL, &ck_blocks);
	if (blocks > 0x7FFFFFFFu || ck_blocks > 0x7FFFFFFFu)
		return ERRV(GENERIC);
	rag_layout(cnt, blocks, J->ck ? &ck_blocks : NULL, &L);
	hb = calloc(1, L.total);
	pass = malloc((size_t)cnt * sizeof(*pass));
	blk = malloc((size_t)(blocks ? blocks : 1u) * sizeof(*blk));
	segs = malloc((size_t)cnt * 4u * sizeof(*segs));
	if (!hb || !pass || !blk || !segs)
		goto out;
	slot0 = segs + cnt;
	gsegs = slot0 + cnt;
	active = gsegs + cnt;
	desc = (struct airs_ragged_desc *)(hb + L.desc);
	dst_off = (uint64_t *)(hb + L.dst_off);
	ids = (uint64_t *)(hb + L.ids);
	row_off = (uint64_t *)(hb + L.row_off);
	caps = (uint32_t *)(hb + L.caps);
	row_len = (uint32_t *)(hb + L.row_len);
	seqs = hb + L.seqs;

	/* the replay; the draws are made below, all of the piece's in table order */
	id = snap.identifier;
	for (j = 0; j < cnt; j++) {
		const uint32_t fb = img->frame_bytes[first + j];
		uint32_t drawn = 0, k;

		if (is_err(engine_prologue(J->ctx, J->frows, J->bound[first + j], fb / sb, &pass[j], &drawn))) {
			*J->ctx = snap; /* the call's eligibility check rules this out */
			goto out;
		}
		J->ctx->sequence_number++;
		for (k = 0; k < drawn; k++)
			id = next_identifier();
		ids[j] = id;
		seqs[j] = pass[j].seq;
	}
	J->ctx->identifier = id;

	/* the geometry: frame rows at 8-byte, sample rows at 16-byte aligned prefix offsets */
	for (j = 0, at = 0; j < cnt; j++) {
		const uint32_t b = J->bound[first + j];

		dst_off[j] = at;
		at += up8(b);
		caps[j] = b;
		max_cap = b > max_cap ? b : max_cap;
		segs[j] = frame_segs(J, first + j);
		slot0[j] = slots;
		slots += segs[j];
	}
	for (j = 0, at = 0; j < cnt; j++) {
		const uint32_t fb = img->frame_bytes[first + j];

		row_off[j] = at;
		if (frame_direct(img, first + j, sb))
			continue;
		row_len[j] = fb;
		at += up16(fb);
		staged++;
		max_len = fb > max_len ? fb : max_len;
	}
	/* the checksum reads what the descriptors below point at: a staged frame's
	 * native row, a direct frame where it lies */
	if (J->ck) {
		uint64_t *ck_src = (uint64_t *)(hb + L.ck_src);
		uint32_t *ck_n = (uint32_t *)(hb + L.ck_n);

		(void)cmp_image_ck_layout(img->frame_bytes + first, sb, cnt, (uint64_t *)(hb + L.ck_off),
					  (struct cmp_image_ck_block *)(hb + L.ck_blocks), NULL);
		for (j = 0; j < cnt; j++) {
			ck_src[j] = row_len[j] ? (uint64_t)(uintptr_t)J->rows + row_off[j]
					       : (uint64_t)(uintptr_t)img->src + img->offsets[first + j];
			ck_n[j] = img->frame_bytes[first + j] / sb;
		}
	}
	/* the launches: the primary pass's frames (sequence number 0), then the secondary's */
	for (g = 0; g < 2; g++) {
		uint64_t nb, i;

		for (j = 0; j < cnt; j++) {
			const int member = (pass[j].seq != 0) == (int)g;

			gsegs[j] = member ? segs[j] : 0u;
			if (member && !gframes[g]++)
				gmember[g] = j;
		}
		if (!gframes[g])
			continue;
		nb = cmp_image_ragged_blocks(gsegs, cnt, active, blk + done);
		for (i = 0; i < nb; i++) {
			struct airs_ragged_desc *d = &desc[done + i];
			const uint32_t fj = blk[done + i].frame;

			d->src = row_len[fj] ? (uint64_t)(uintptr_t)J->rows + row_off[fj]
					     : (uint64_t)(uintptr_t)img->src + img->offsets[first + fj];
			d->n = img->frame_bytes[first + fj] / sb;
			d->seg = blk[done + i].seg;
			d->frame = fj;
			d->slot0 = slot0[fj];
		}
		gfirst[g] = done;
		gblocks[g] = nb;
		done += nb;
	}
	if (airs_dev_h2d(J->dev, J->rag, hb, L.total))
		goto out;
	if (staged) {
		struct airs_encode_image q;

		memset(&q, 0, sizeof(q));
		q.stage = AIRS_ENCIMG_INGEST;
		q.count = cnt;
		q.src = img->src;
		q.offsets = J->d_off + first;
		q.frame_bytes = max_len;
		q.swap = (img->flags & CMP_GPU_IMG_SRC_BIG_ENDIAN) != 0;
		q.rows = J->rows;
		q.row_off = (const uint64_t *)(J->rag + L.row_off);
		q.row_len = (const uint32_t *)(J->rag + L.row_len);
		q.staged = staged;
		e = airs_dev_encode_image(J->dev, &q);
		if (e)
			goto out;
	}
	/* one XXH32 launch pair for the frames of both passes: it does not depend on the pass */
	if (J->ck) {
		struct airs_ragged_ck c;

		memset(&c, 0, sizeof(c));
		c.sample_bytes = sb;
		c.frames = cnt;
		c.src = (const uint64_t *)(J->rag + L.ck_src);
		c.n = (const uint32_t *)(J->rag + L.ck_n);
		c.off = (const uint64_t *)(J->rag + L.ck_off);
		c.bytes = ck_bytes;
		c.blocks = (const struct airs_ragged_ck_block *)(J->rag + L.ck_blocks);
		c.num_blocks = (uint32_t)ck_blocks;
		c.out = (uint32_t *)(J->rag + L.ck_out);
		e = airs_dev_checksum_ragged(J->dev, &c);
		if (e)
			goto out;
	}
	for (g = 0; g < 2; g++) {
		const struct pass *p = &pass[gmember[g]];
		struct airs_ragged r;

		if (!gframes[g])
			continue;
		memset(&r, 0, sizeof(r));
		r.sample_bytes = sb;
		r.frames = gframes[g];
		r.blocks = (uint32_t)gblocks[g];
		r.slots = slots;
		r.desc = (const struct airs_ragged_desc *)(J->rag + L.desc) + gfirst[g];
		r.dst = J->frows;
		r.dst_off = (const uint64_t *)(J->rag + L.dst_off);
		r.caps = (const uint32_t *)(J->rag + L.caps);
		r.ids = (const uint64_t *)(J->rag + L.ids);
		r.seqs = J->rag + L.seqs;
		r.preprocessing = p->pre;
		r.encoder_type = p->enc;
		r.encoder_param = p->par;
		r.outlier_param = p->outlier_param;
		r.status = img->sizes + first;
		r.checksums = J->ck ? (const uint32_t *)(J->rag + L.ck_out) : NULL;
		e = airs_dev_encode_ragged(J->dev, &r);
		if (e)
			goto out;
	}
	e = piece_emit(J, first, cnt, max_cap, (const uint64_t *)(J->rag + L.dst_off), 0);
out:
	free(hb);
	free(pass);
	free(blk);
	free(segs);
	return e;
}

/* The ragged path applies: the option is on, the frames of the context are
 * independent (no state in the work buffer), no frame can fall back, a
 * checksum has been opted in (CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM: the pieces
 * then take the ragged XXH32), nothing needs the batch path's flags, and the
 * context's passes are ones the prologue accepts (tried on a copy, with the
 * draws only counted). */
static int ragged_applies(const struct image_job *J)
{
	const struct cmp_params *P = &J->ctx->params;
	struct cmp_context c = *J->ctx;
	struct pass p;
	uint32_t drawn = 0;
	uint64_t dummy[4];

	if (!J->engine->image_ragged || work_buf_state(P) || (P->checksum_enabled && !J->engine->image_ragged_ck) ||
	    P->uncompressed_fallback_enabled || J->img->batch_flags)
		return 0;
	c.sequence_number = 0;
	if (is_err(engine_prologue(&c, dummy, HDR_MAX_SIZE, 1, &p, &drawn)))
		return 0;
	c.sequence_number = 1;
	if (P->secondary_iterations && is_err(engine_prologue(&c, dummy, HDR_MAX_SIZE, 1, &p, &drawn)))
		return 0;
	return 1;
}

uint32_t cmp_gpu_compress_image(struct cmp_gpu_engine *engine, struct cmp_context *ctx,
				const struct cmp_gpu_encode_image *img)
{
	struct image_job J;
	struct cmp_image_piece p;
	uint64_t f, N;
	size_t rows_bytes = 0, frows_bytes = 0, rag_bytes = 0, rag_at;
	uint32_t sample_bytes, e = 0, staged = 0;

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
	sample_bytes = img->type == CMP_GPU_I16_IN_I32 ? 4u : 2u;
	memset(&J, 0, sizeof(J));
	J.engine = engine;
	J.dev = engine->dev;
	J.ctx = ctx;
	J.img = img;
	J.sample_bytes = sample_bytes;
	J.first_run = 1;
	if (ragged_applies(&J)) {
		J.bound = malloc((size_t)N * sizeof(*J.bound));
		if (!J.bound)
			return ERRV(GENERIC);
		for (f = 0; f < N; f++)
			(void)frame_refusal(img->frame_bytes[f], sample_bytes, &J.bound[f]);
		J.keep = engine->image_ragged == 1u ? CMP_IMAGE_RAGGED_KEEP : engine->image_ragged;
		J.seg = airs_dev_ragged_segment(sample_bytes);
		J.ck = ctx->params.checksum_enabled != 0;
	}

	/* the rows and tables of the largest piece, allocated once: growing them
	 * between pieces would wait for the stream */
	for (f = 0; f < N; f += p.count) {
		size_t need = 0, srows = 0;
		uint64_t stride, blocks = 0;
		uint32_t j;

		next_piece(&J, f, &p);
		if (p.kind == CMP_IMAGE_PIECE_REFUSED)
			continue;
		if (p.kind == CMP_IMAGE_PIECE_RUN) {
			const uint32_t fb = img->frame_bytes[f];

			need = (size_t)p.count * up8(cmp_compress_bound(fb));
			if (!run_direct(img, f, p.count, sample_bytes, &stride))
				srows = (size_t)p.count * up16(fb);
		} else {
			struct rag_layout L;
			uint64_t ck_blocks = 0;

			for (j = 0; j < p.count; j++) {
				need += up8(J.bound[f + j]);
				blocks += frame_segs(&J, f + j);
				if (!frame_direct(img, f + j, sample_bytes))
					srows += up16(img->frame_bytes[f + j]);
			}
			if (J.ck)
				(void)cmp_image_ck_layout(img->frame_bytes + f, sample_bytes, p.count, NULL, NULL, &ck_blocks);
			rag_layout(p.count, blocks, J.ck ? &ck_blocks : NULL, &L);
			rag_bytes = L.total > rag_bytes ? L.total : rag_bytes;
		}
		frows_bytes = need > frows_bytes ? need : frows_bytes;
		staged |= srows != 0;
		rows_bytes = srows > rows_bytes ? srows : rows_bytes;
	}
	/* the sticky word, then the offsets of the frames in src, then a ragged piece's tables */
	rag_at = (8u + (staged ? (size_t)N * 8u : 0u) + 31u) & ~(size_t)31u;
	J.tables = airs_dev_scratch(J.dev, AIRS_SLOT_ENCIMG, rag_at + rag_bytes);
	J.frows = airs_dev_scratch(J.dev, AIRS_SLOT_ENCIMG + 2, frows_bytes + 16u);
	if (staged)
		J.rows = airs_dev_scratch(J.dev, AIRS_SLOT_ENCIMG + 1, rows_bytes);
	if (!J.tables || !J.frows || (staged && !J.rows)) {
		free(J.bound);
		return ERRV(GENERIC);
	}
	J.d_off = (uint64_t *)(J.tables + 8u);
	J.rag = J.tables + rag_at;
	/* Straight from the caller's pageable table, as the batch path uploads its
	 * identifiers (cmp_batch.c): the runtime has staged a pageable source when
	 * the copy call returns.  The engine's page-locked scratch is no place for
	 * it: this call does not wait, and the next call on the engine may rewrite
	 * that scratch while the copy is still queued. */
	if (staged && airs_dev_h2d(J.dev, J.d_off, img->offsets, (size_t)N * 8u)) {
		free(J.bound);
		return ERRV(GENERIC);
	}

	for (f = 0, e = 0; f < N && !e; f += p.count) {
		next_piece(&J, f, &p);
		e = p.kind == CMP_IMAGE_PIECE_RAGGED ? piece_ragged(&J, f, p.count) : piece_run(&J, f, p.count);
	}
	free(J.bound);
	return e;
}
