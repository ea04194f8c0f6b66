/*
 * cmp_estimate.c -- cmp_gpu_estimate and cmp_gpu_estimate_frame_size
 * (include/cmp_gpu.h): the exact payload bits of every frame of a batch under
 * up to 64 parameter sets (estimate.hip).  The encoder arguments of every
 * candidate are resolved by the encoder's own checks (cmp_coder_resolve,
 * cmp_host.c) into the table the device layer sizes with.  The call-level
 * validation returns before anything touches the device.
 */
#include <stdint.h>
#include <string.h>

#include "cmp.h"
#include "cmp_errors.h"
#include "cmp_header.h"
#include "cmp_gpu.h"
#include "airs_dev.h"
#include "airs_rcp.h"
#include "cmp_engine.h"

#define ERRV(name) ((uint32_t)0u - (uint32_t)CMP_ERR_##name)
#define HDR_MAX_SIZE 22u /* a header with the encoder fields (cmp_header.h) */

/* header bytes of a frame coded with c (cmp_host.c, the pass plan) */
static uint32_t header_bytes(const struct cmp_gpu_candidate *c)
{
	return c->preprocessing == CMP_PREPROCESS_NONE && c->encoder_type == CMP_ENCODER_UNCOMPRESSED
		       ? (uint32_t)CMP_HDR_SIZE
		       : HDR_MAX_SIZE;
}

uint32_t cmp_gpu_estimate_frame_size(const struct cmp_gpu_candidate *c, uint64_t bits, int checksum_enabled)
{
	uint32_t e;
	uint64_t payload, size;

	if (!c)
		return ERRV(GENERIC);
	e = cmp_coder_resolve(c->encoder_type, c->encoder_param, c->encoder_outlier, NULL);
	if (e > ERRV(MAX_CODE))
		return e;
	payload = bits / 8u + (bits % 8u ? 1u : 0u);
	size = header_bytes(c) + (checksum_enabled ? (uint64_t)CMP_CHECKSUM_SIZE : 0u);
	if (payload > CMP_HDR_MAX_COMPRESSED_SIZE || size + payload > CMP_HDR_MAX_COMPRESSED_SIZE)
		return ERRV(HDR_CMP_SIZE_TOO_LARGE);
	return (uint32_t)(size + payload);
}

uint32_t cmp_gpu_estimate(struct cmp_gpu_engine *engine, const struct cmp_gpu_estimate_batch *batch)
{
	struct airs_est_cand tab[CMP_GPU_ESTIMATE_MAX_CANDIDATES];
	struct airs_estimate q;
	uint32_t bytes, n, c;

	if (!engine || !batch || !batch->candidates || !batch->bits)
		return ERRV(GENERIC);
	if (batch->num_frames == 0 || batch->num_frames > CMP_GPU_ESTIMATE_MAX_FRAMES)
		return ERRV(GENERIC);
	if (batch->num_candidates == 0 || batch->num_candidates > CMP_GPU_ESTIMATE_MAX_CANDIDATES)
		return ERRV(GENERIC);
	if (batch->flags || (uint32_t)batch->type > (uint32_t)CMP_GPU_I16_IN_I32 || ((uintptr_t)batch->bits & 7u) ||
	    ((uintptr_t)batch->best & 3u))
		return ERRV(GENERIC);
	bytes = batch->type == CMP_GPU_I16_IN_I32 ? 4u : 2u;
	if (!batch->src)
		return ERRV(SRC_NULL);
	if ((uintptr_t)batch->src & (bytes - 1u))
		return ERRV(GENERIC);
	if (batch->src_size == 0 || batch->src_size % bytes)
		return ERRV(SRC_SIZE_WRONG);
	n = batch->src_size / bytes;
	if ((uint64_t)n * 2u > CMP_HDR_MAX_ORIGINAL_SIZE)
		return ERRV(HDR_ORIGINAL_TOO_LARGE);
	if (batch->num_frames > 1 && (batch->src_stride < batch->src_size || batch->src_stride % bytes))
		return ERRV(GENERIC);
	memset(tab, 0, sizeof(tab));
	for (c = 0; c < batch->num_candidates; c++) {
		const struct cmp_gpu_candidate *u = &batch->candidates[c];
		struct airs_est_cand *t = &tab[c];
		uint32_t e, g = u->encoder_param;

		if ((uint32_t)u->preprocessing > (uint32_t)CMP_PREPROCESS_MODEL)
			return ERRV(PARAMS_INVALID);
		/* the encoder's own checks (encoder.c:185-224) */
		e = cmp_coder_resolve(u->encoder_type, g, u->encoder_outlier, &t->outlier);
		if (e > ERRV(MAX_CODE))
			return e;
		if (u->preprocessing == CMP_PREPROCESS_MODEL &&
		    (!batch->model || ((uintptr_t)batch->model & 1u) || (batch->model_stride & 1u) ||
		     (batch->num_frames > 1 && batch->model_stride < 2ull * n)))
			return ERRV(PARAMS_INVALID);
		t->pre = (uint32_t)u->preprocessing;
		t->hdr = header_bytes(u);
		if (u->encoder_type == CMP_ENCODER_UNCOMPRESSED) {
			t->kind = AIRS_EST_RAW;
			continue;
		}
		while ((2u << t->k) <= g)
			t->k++;
		t->cutoff = (2u << t->k) - g;
		t->g = g;
		t->rcp = airs_rcp_u32(g, 65537u); /* dividends are at most 65536: non-zero for every g */
		if (u->encoder_type == CMP_ENCODER_GOLOMB_MULTI)
			t->kind = AIRS_EST_MULTI;
		else
			t->kind = (g & (g - 1u)) == 0u ? AIRS_EST_ZERO_P2 : AIRS_EST_ZERO;
	}
	memset(&q, 0, sizeof(q));
	q.src = batch->src;
	q.src_stride = batch->src_stride;
	q.sample_bytes = bytes;
	q.n = n;
	q.num_frames = batch->num_frames;
	q.model = batch->model;
	q.model_stride = batch->model_stride;
	q.cand = tab;
	q.num_cand = batch->num_candidates;
	q.bits = batch->bits;
	q.best = batch->best;
	return airs_dev_estimate(engine->dev, &q);
}
