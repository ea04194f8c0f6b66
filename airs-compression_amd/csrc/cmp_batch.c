/*
 * cmp_batch.c -- the batch planner behind cmp_gpu_compress (cmp_gpu.h): what a
 * batch of frames of many contexts becomes on the device.  The context state
 * machine is the cmp.h engine's (cmp_host.c, through cmp_pass.h); this file
 * decides the route, builds the launches and commits
 * the identifiers and the contexts' state.  All device work goes through
 * airs_dev.h.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cmp_engine.h"
#include "cmp_pass.h"

#define IWT_SCRATCH_MAX (1ull << 30) /* device scratch batch_iwt may take for coefficients */
/* cmp_gpu_batch.draws is written only when the caller asks for it (ADVICE r3:
 * a caller that fills the struct field by field may leave it uninitialised) */
#define REPORT_DRAWS(b) (((b)->flags & CMP_GPU_REPORT_DRAWS) && (b)->draws)

/* per-frame plan of a batch, computed by replaying the context state machine */
struct frame_plan {
	struct pass p;
	uint64_t id;
};

/* what every route is handed: the call's arguments, the shape of its frames,
 * and host scratch [sh.total]: the plan, identifiers, staging for pointers */
struct batch_job {
	struct airs_dev_engine *dev;
	struct cmp_context *ctx;
	uint32_t num_ctx, fpc;
	const struct cmp_gpu_batch *b;
	struct batch_shape sh;
	struct frame_plan *plan;
	uint64_t *ids, *ptrs;
};

static int same_pass(const struct pass *a, const struct pass *b)
{
	return a->pre == b->pre && a->enc == b->enc && a->par == b->par &&
	       a->outlier_param == b->outlier_param && a->model_mode == b->model_mode && a->seq == b->seq;
}

/* this pass takes per-frame Rice selection under CMP_GPU_AUTO_RICE */
static int pass_auto_rice(const struct pass *p)
{
	return p->enc == CMP_ENCODER_GOLOMB_ZERO &&
	       (p->pre == CMP_PREPROCESS_NONE || p->pre == CMP_PREPROCESS_DIFF || p->pre == CMP_PREPROCESS_IWT);
}

/* is v[j] = v[0] + j*step for all j?  (step returned) */
static int affine_u64(const uint64_t *v, uint32_t cnt, uint64_t *step)
{
	uint32_t j;

	*step = cnt > 1 ? v[1] - v[0] : 0;
	for (j = 2; j < cnt; j++)
		if (v[j] - v[j - 1] != *step)
			return 0;
	return 1;
}

/* a frame of this context that does not fit falls back to raw storage (cmp.c:358-366) */
static int fallback_applies(const struct cmp_context *ctx, const struct cmp_gpu_batch *b, uint32_t n)
{
	return ctx->params.uncompressed_fallback_enabled && b->dst_capacity >= raw_frame_size(ctx, n);
}

/* first-attempt capacity of a frame (cmp_compress_generic, cmp.c:358-366) */
static uint32_t first_cap(const struct cmp_context *ctx, const struct cmp_gpu_batch *b, uint32_t n)
{
	return fallback_applies(ctx, b, n) ? raw_frame_size(ctx, n) : b->dst_capacity;
}

/* where the work buffers of ctx[0..k) lie: strided (context c's at base +
 * c * stride; stride is ctx[1]'s distance from ctx[0] either way), or else a
 * pointer list is needed (upload_model_ptrs); al16: all 16-byte aligned */
struct model_addr {
	void *base;
	uint64_t stride;
	uint32_t strided, al16;
};

static struct model_addr model_addressing(const struct cmp_context *ctx, uint32_t k)
{
	const uint64_t base = (uint64_t)(uintptr_t)ctx[0].work_buf;
	struct model_addr m = { ctx[0].work_buf, 0, 1, 1 };
	uint32_t c;

	if (k > 1)
		m.stride = (uint64_t)(uintptr_t)ctx[1].work_buf - base;
	for (c = 0; c < k; c++) {
		if ((uint64_t)(uintptr_t)ctx[c].work_buf != base + c * m.stride)
			m.strided = 0;
		if ((uintptr_t)ctx[c].work_buf & 15u)
			m.al16 = 0;
	}
	return m;
}

/* A pointer list into SLOT_AUX: ptrs[0..cnt) as the caller filled it (one per
 * launch frame), or with ctx given the work buffers of ctx[0..cnt), staged in
 * ptrs.  The copy is asynchronous: ptrs stays as it is until the caller has
 * synchronised.  Returns the device list or NULL. */
static const uint64_t *upload_model_ptrs(struct airs_dev_engine *dev, const struct cmp_context *ctx, uint64_t *ptrs,
					 uint32_t cnt)
{
	uint64_t *d_ptr = airs_dev_scratch(dev, SLOT_AUX, (size_t)cnt * 8u);
	uint32_t j;

	for (j = 0; ctx && j < cnt; j++)
		ptrs[j] = (uint64_t)(uintptr_t)ctx[j].work_buf;
	if (!d_ptr || is_err(airs_dev_h2d(dev, d_ptr, ptrs, (size_t)cnt * 8u)))
		return NULL;
	return d_ptr;
}

/* Launch cnt frames that share one pass: launch frame j is batch frame
 * fl[j] (host list) or add + j*mul; output capacity cap.  coef: J->ptrs[j]
 * holds the work buffer of launch frame j, in place of its context's (IWT
 * frames of one context in one launch, batch_iwt). */
static uint32_t batch_launch(const struct batch_job *J, const uint32_t *fl, uint32_t add, uint32_t mul, uint32_t cnt,
			     uint32_t cap, int coef)
{
	struct airs_dev_engine *dev = J->dev;
	const struct cmp_gpu_batch *b = J->b;
	const uint32_t fpc = J->fpc, f0 = fl ? fl[0] : add;
	const struct pass *P = &J->plan[f0].p;
	uint32_t nframes_total = 0;
	struct airs_launch L;
	uint64_t step;
	uint32_t j, e, *d_ck = NULL, *d_fl = NULL;

#define FRAME_AT(jj) (fl ? fl[jj] : add + (jj) * mul)
	launch_fill(&L, b, &J->sh, &J->ctx[f0 / fpc], P, cap);
	if (fl) {
		/* an affine list launches without a device copy */
		uint32_t aff = 1, m = cnt > 1 ? fl[1] - fl[0] : 1;

		for (j = 1; j < cnt && aff; j++)
			aff = fl[j] == fl[0] + j * m;
		if (aff) {
			add = fl[0];
			mul = m;
			fl = NULL;
		}
	}
	for (j = 0; j < cnt; j++) {
		const uint32_t f = FRAME_AT(j);

		J->ids[j] = J->plan[f].id;
		if (f + 1u > nframes_total)
			nframes_total = f + 1u;
	}
	if (fl) {
		d_fl = airs_dev_scratch(dev, SLOT_FL, (size_t)cnt * 4u);
		if (!d_fl || is_err(airs_dev_h2d(dev, d_fl, fl, (size_t)cnt * 4u)) || is_err(airs_dev_sync(dev)))
			return ERRV(GENERIC);
	}
	if (affine_u64(J->ids, cnt, &step)) {
		L.id_base = J->ids[0];
		L.id_step = step;
	} else {
		uint64_t *d_ids = airs_dev_scratch(dev, SLOT_IDS, (size_t)cnt * 8u);

		if (!d_ids || is_err(airs_dev_h2d(dev, d_ids, J->ids, (size_t)cnt * 8u)) || is_err(airs_dev_sync(dev)))
			return ERRV(GENERIC);
		L.ids = d_ids;
	}
	if (P->model_mode != AIRS_MODEL_NONE || P->pre == CMP_PREPROCESS_IWT) {
		struct model_addr m = { NULL, 0, 0, 0 };

		if (!coef) /* the contexts up to the launch's last frame */
			m = model_addressing(J->ctx, (nframes_total + fpc - 1) / fpc);
		if (m.strided) {
			/* model of frame f = base + (f / fpc) * stride */
			L.model = m.base;
			L.model_stride = m.stride;
			L.model_div = fpc;
		} else {
			L.model_ptrs_al16 = 1;
			for (j = 0; j < cnt; j++) {
				if (!coef)
					J->ptrs[j] = (uint64_t)(uintptr_t)J->ctx[FRAME_AT(j) / fpc].work_buf;
				if (J->ptrs[j] & 15u)
					L.model_ptrs_al16 = 0;
			}
			L.model_ptrs = upload_model_ptrs(dev, NULL, J->ptrs, cnt);
			if (!L.model_ptrs || is_err(airs_dev_sync(dev)))
				return ERRV(GENERIC);
		}
	}
#undef FRAME_AT
	if (L.checksum_enabled) {
		d_ck = airs_dev_scratch(dev, SLOT_CK, (size_t)nframes_total * 4u);
		if (!d_ck)
			return ERRV(GENERIC);
		if (fl)
			e = airs_dev_checksum(dev, b->src, b->src_stride, L.sample_bytes, L.n, cnt, d_fl, d_ck);
		else if (mul == 1)
			e = airs_dev_checksum(dev, (const uint8_t *)b->src + (uint64_t)add * b->src_stride,
					      b->src_stride, L.sample_bytes, L.n, cnt, NULL, d_ck + add);
		else
			e = airs_dev_checksum(dev, b->src, b->src_stride, L.sample_bytes, L.n, nframes_total, NULL, d_ck);
		if (is_err(e))
			return e;
	}
	if ((b->flags & CMP_GPU_AUTO_RICE) && pass_auto_rice(P)) {
		L.frame_g_scratch = airs_dev_scratch(dev, SLOT_G, (size_t)nframes_total * 4u);
		if (!L.frame_g_scratch)
			return ERRV(GENERIC);
		L.auto_rice = 1;
	}
	L.num_frames = cnt;
	L.frame_list = d_fl;
	L.frame_add = add;
	L.frame_mul = mul;
	L.checksums = d_ck;
	return airs_dev_encode(dev, &L);
}

/* host scratch of the step-by-step paths, one allocation (id0 owns it): arrays
 * [num_ctx], and the identifier draws of every frame [total] */
struct step_scratch {
	uint64_t *id0;                   /* the identifiers the contexts came with */
	uint32_t *list, *caps, *grp;     /* frames to launch and their capacities; one launch's frames */
	uint32_t *sz;                    /* a step's frame sizes (or errors) by context */
	uint8_t *done, *draws;
};

static int step_scratch_alloc(struct step_scratch *s, uint32_t num_ctx, uint32_t total)
{
	const size_t k = num_ctx;

	s->id0 = calloc(1, k * (8u + 4u * 4u + 1u) + total);
	if (!s->id0)
		return 0;
	s->list = (uint32_t *)(s->id0 + k);
	s->caps = s->list + k;
	s->grp = s->caps + k;
	s->sz = s->grp + k;
	s->done = (uint8_t *)(s->sz + k);
	s->draws = s->done + k;
	return 1;
}

/* launch the cnt frames of s->list (batch frames of one acquisition step): one
 * launch per run of frames with the same pass and capacity */
static uint32_t launch_groups(const struct batch_job *J, struct step_scratch *s, uint32_t cnt)
{
	const struct cmp_context *ctx = J->ctx;
	const uint32_t *list = s->list, *caps = s->caps;
	const uint32_t fpc = J->fpc;
	uint32_t i, k, e = 0;

	memset(s->done, 0, cnt);
	for (i = 0; i < cnt && !is_err(e); i++) {
		uint32_t g = 0;

		if (s->done[i])
			continue;
		for (k = i; k < cnt; k++) {
			if (!s->done[k] && caps[k] == caps[i] && same_pass(&J->plan[list[k]].p, &J->plan[list[i]].p) &&
			    ctx[list[k] / fpc].params.model_rate == ctx[list[i] / fpc].params.model_rate &&
			    ctx[list[k] / fpc].params.checksum_enabled == ctx[list[i] / fpc].params.checksum_enabled &&
			    /* launch_fill decides the model fail bit from the
			     * launch's first context: one fallback setting per launch */
			    !ctx[list[k] / fpc].params.uncompressed_fallback_enabled ==
				    !ctx[list[i] / fpc].params.uncompressed_fallback_enabled) {
				s->grp[g++] = list[k];
				s->done[k] = 1;
			}
		}
		e = batch_launch(J, s->grp, 0, 1, g, caps[i], 0);
	}
	return e;
}

/* launch the cnt frames of s->list, read their sizes back (s->sz, by context) */
static uint32_t step_run(const struct batch_job *J, struct step_scratch *s, uint32_t cnt)
{
	uint32_t k, e = launch_groups(J, s, cnt);

	for (k = 0; k < cnt && !is_err(e); k++)
		e = airs_dev_d2h(J->dev, &s->sz[s->list[k] / J->fpc], J->b->sizes + s->list[k], 4u);
	return is_err(e) ? e : airs_dev_sync(J->dev);
}

/* Draw the identifiers of a batch in the reference's call order
 * (context-major): frame f draws draws[f] identifiers and carries the last
 * one; a frame without a draw carries its context's, which is
 * from[c].identifier at the context's first frame.  report (optional)
 * receives the draw counts. */
static void draw_identifiers(const struct cmp_context *from, uint32_t num_ctx, uint32_t fpc, const uint8_t *draws,
			     uint64_t *ids, uint8_t *report)
{
	uint32_t c, a, k;

	for (c = 0; c < num_ctx; c++) {
		uint64_t id = from[c].identifier;

		for (a = 0; a < fpc; a++) {
			const uint32_t f = c * fpc + a;

			for (k = 0; k < draws[f]; k++)
				id = next_identifier();
			ids[f] = id;
			if (report)
				report[f] = draws[f];
		}
	}
}

/* How the drawn identifiers (J->ids) reach the headers of the batch's frames
 * (frames whose size is an error value keep theirs).  pinned: page-locked
 * staging for the identifiers (not for COMMIT_SYNC). */
enum commit_how {
	COMMIT_SYNC,   /* pageable upload to SLOT_IDS, patch, synchronise */
	COMMIT_ASYNC,  /* staged in pinned; upload to SLOT_IDS and patch, both asynchronous */
	COMMIT_DIRECT  /* staged in pinned, which the patch reads over the bus; asynchronous */
};

static uint32_t commit_ids(const struct batch_job *J, enum commit_how how, uint64_t *pinned)
{
	const size_t bytes = (size_t)J->sh.total * 8u;
	const uint64_t *from = J->ids;
	uint32_t e;

	if (how != COMMIT_SYNC)
		from = memcpy(pinned, J->ids, bytes);
	if (how != COMMIT_DIRECT) {
		uint64_t *d_ids = airs_dev_scratch(J->dev, SLOT_IDS, bytes);

		if (!d_ids || is_err(airs_dev_h2d(J->dev, d_ids, from, bytes)))
			return ERRV(GENERIC);
		from = d_ids;
	}
	e = airs_dev_patch_ids(J->dev, J->b->dst, J->b->dst_stride, J->sh.total, 0, 1, from, J->b->sizes);
	if (!is_err(e) && how == COMMIT_SYNC)
		e = airs_dev_sync(J->dev);
	return e;
}

static void ctx_commit(struct cmp_context *ctx, uint64_t id, uint32_t seq, uint32_t model_size)
{
	ctx->identifier = id;
	ctx->sequence_number = (uint8_t)seq;
	ctx->model_size = model_size;
}

/*
 * Exact mode: one acquisition step at a time, as the host API would run it.
 * Used when a frame can fail or fall back to raw storage, because the
 * outcome of frame (c, a) decides the pass (and identifier draws) of frame
 * (c, a+1).  Per step: plan every context, launch, read the sizes back, run
 * the fallback frames (cmp_compress_generic: reset, NONE + UNCOMPRESSED at
 * the raw size), and advance the contexts that succeeded.  Identifier draws
 * are counted per frame and made at the end in the reference's call order
 * (context-major), then written into the headers.
 */
static uint32_t batch_exact(const struct batch_job *J)
{
	struct airs_dev_engine *dev = J->dev;
	struct cmp_context *ctx = J->ctx;
	const struct cmp_gpu_batch *b = J->b;
	const uint32_t num_ctx = J->num_ctx, fpc = J->fpc, n = J->sh.n;
	struct step_scratch s;
	uint32_t a, c, e = 0;

	if (!step_scratch_alloc(&s, num_ctx, J->sh.total))
		return ERRV(GENERIC);
	for (c = 0; c < num_ctx; c++)
		s.id0[c] = ctx[c].identifier;
	for (a = 0; a < fpc && !is_err(e); a++) {
		uint32_t nl = 0;

		for (c = 0; c < num_ctx && !is_err(e); c++) {
			const uint32_t f = c * fpc + a, cap = first_cap(&ctx[c], b, n);
			void *dst = (uint8_t *)b->dst + (uint64_t)f * b->dst_stride;
			uint32_t drawn = 0;

			s.sz[c] = engine_prologue(&ctx[c], dst, cap, n, &J->plan[f].p, &drawn);
			s.draws[f] = (uint8_t)drawn;
			J->plan[f].id = 0; /* written at the end */
			if (is_err(s.sz[c])) { /* a frame the host API rejects before encoding keeps its error */
				e = airs_dev_h2d(dev, b->sizes + f, &s.sz[c], 4u);
			} else {
				s.list[nl] = f;
				s.caps[nl++] = cap;
			}
		}
		if (is_err(e) || is_err(e = step_run(J, &s, nl)))
			break;
		for (c = 0, nl = 0; c < num_ctx && !is_err(e); c++) {
			const uint32_t f = c * fpc + a, raw = raw_frame_size(&ctx[c], n);
			void *dst = (uint8_t *)b->dst + (uint64_t)f * b->dst_stride;
			uint32_t drawn = 0;

			/* sz[c] holds the prologue's error when the frame was rejected
			 * before encoding (e.g. raw size below the compressed header) */
			if (!(fallback_applies(&ctx[c], b, n) && cmp_get_error_code(s.sz[c]) == CMP_ERR_DST_TOO_SMALL))
				continue;
			/* cmp.c:342-393: reset, then the frame again as NONE + UNCOMPRESSED */
			s.sz[c] = fallback_prologue(&ctx[c], dst, raw, n, &J->plan[f].p, &drawn);
			s.draws[f] = (uint8_t)(s.draws[f] + drawn);
			if (is_err(s.sz[c])) {
				e = airs_dev_h2d(dev, b->sizes + f, &s.sz[c], 4u);
				continue;
			}
			s.list[nl] = f;
			s.caps[nl++] = raw;
		}
		if (is_err(e) || (nl && is_err(e = step_run(J, &s, nl))))
			break;
		for (c = 0; c < num_ctx; c++)
			if (!is_err(s.sz[c]))
				ctx[c].sequence_number++;
	}
	if (!is_err(e)) {
		/* identifiers in call order; the resets cleared the contexts', and a
		 * frame before its context's first draw carries the one it came with */
		for (c = 0; c < num_ctx; c++)
			ctx[c].identifier = s.id0[c];
		draw_identifiers(ctx, num_ctx, fpc, s.draws, J->ids, REPORT_DRAWS(b) ? b->draws : NULL);
		for (c = 0; c < num_ctx; c++)
			ctx[c].identifier = J->ids[c * fpc + fpc - 1u];
		e = commit_ids(J, COMMIT_SYNC, NULL);
	}
	free(s.id0);
	return e;
}

/*
 * Exact mode on the device.  When every context has the same parameters and
 * the prologue's static checks pass for both passes, the state machine
 * that batch_exact() steps on the host runs on the GPU instead
 * (airs_dev_fb_step / airs_dev_fb_copy, airs_dev.h): per acquisition step a
 * planning kernel, the primary-pass launch, the secondary-pass launch (holes
 * in their frame lists skip the contexts on the other pass) and the raw
 * frames of the previous step's fallbacks.  The only host round trip is one
 * read-back of the identifier draw counts and context states at the end;
 * identifiers are then drawn in call order and patched into the headers.
 */
static int same_params(const struct cmp_params *x, const struct cmp_params *y)
{
	return x->primary_preprocessing == y->primary_preprocessing &&
	       x->primary_encoder_type == y->primary_encoder_type &&
	       x->primary_encoder_param == y->primary_encoder_param &&
	       x->primary_encoder_outlier == y->primary_encoder_outlier &&
	       x->secondary_iterations == y->secondary_iterations &&
	       x->secondary_preprocessing == y->secondary_preprocessing &&
	       x->secondary_encoder_type == y->secondary_encoder_type &&
	       x->secondary_encoder_param == y->secondary_encoder_param &&
	       x->secondary_encoder_outlier == y->secondary_encoder_outlier && x->model_rate == y->model_rate &&
	       x->checksum_enabled == y->checksum_enabled &&
	       x->uncompressed_fallback_enabled == y->uncompressed_fallback_enabled;
}

/* checksums of all frames of the batch into SLOT_CK (*d_ck) */
static uint32_t batch_checksums(const struct batch_job *J, const uint32_t **d_ck)
{
	uint32_t *ck = airs_dev_scratch(J->dev, SLOT_CK, (size_t)J->sh.total * 4u);

	*d_ck = ck;
	if (!ck)
		return ERRV(GENERIC);
	return airs_dev_checksum(J->dev, J->b->src, J->b->src_stride, J->sh.bytes, J->sh.n, J->sh.total, NULL, ck);
}

/* can batch_device_exact() run this batch?  pp / ps receive the two passes */
static int device_exact_ok(const struct batch_job *J, struct pass *pp, struct pass *ps)
{
	const struct cmp_context *ctx = J->ctx;
	const struct cmp_params *P = &ctx[0].params;
	const uint32_t n = J->sh.n;
	uint32_t c, sq, draws = 0;

	memset(ps, 0, sizeof(*ps));
	for (c = 0; c < J->num_ctx; c++) {
		if (!same_params(&ctx[c].params, P))
			return 0;
		/* a first frame (sequence number 0), then a secondary one: equal
		 * parameters resolve to equal passes, so every context writes them */
		for (sq = 0; sq < (P->secondary_iterations ? 2u : 1u); sq++) {
			struct cmp_context t = ctx[c];

			t.sequence_number = (uint8_t)sq;
			if (sq)
				t.model_size = 2u * n;
			if (is_err(engine_prologue(&t, J->b->dst, first_cap(&ctx[c], J->b, n), n, sq ? ps : pp, &draws)))
				return 0;
		}
	}
	return 1;
}

static uint32_t batch_device_exact(const struct batch_job *J, const struct pass *pp, const struct pass *ps)
{
	struct airs_dev_engine *dev = J->dev;
	struct cmp_context *ctx = J->ctx;
	const struct cmp_gpu_batch *b = J->b;
	const struct cmp_params *P = &ctx[0].params;
	const uint32_t num_ctx = J->num_ctx, fpc = J->fpc, n = J->sh.n, total = J->sh.total;
	const uint32_t cap1 = first_cap(&ctx[0], b, n);
	const size_t words = 4u * (size_t)num_ctx, tb = ((size_t)total + 15u) & ~(size_t)15u;
	uint32_t *host_state = calloc(1, 8u * (size_t)num_ctx + total); /* then the draws */
	uint8_t *host_draws = (uint8_t *)(host_state + 2u * (size_t)num_ctx);
	uint8_t *scr = airs_dev_scratch(dev, SLOT_FL, words * 4u + 4u * tb);
	struct model_addr m = { NULL, 0, 0, 0 }; /* the work buffers: the model, or IWT coefficients */
	uint32_t *d_g = NULL, c, a, e = 0;
	struct airs_fb_step S;

	if (!host_state || !scr) {
		e = ERRV(GENERIC);
		goto out;
	}
	memset(&S, 0, sizeof(S));
	S.state = (uint32_t *)scr;
	S.flist_p = S.state + 2u * num_ctx;
	S.flist_s = S.flist_p + num_ctx;
	S.seqs = scr + words * 4u;
	S.draws = S.seqs + tb;
	S.kind = S.draws + tb;
	S.fb = S.kind + tb;
	S.num_ctx = num_ctx;
	S.fpc = fpc;
	S.packed = 2u * n;
	S.iters = P->secondary_iterations;
	S.model_needed = model_needed(P) ? 1u : 0u;
	S.raw_size = raw_frame_size(&ctx[0], n);
	S.fb_eligible = fallback_applies(&ctx[0], b, n);
	S.err_floor = ERRV(MAX_CODE);
	S.err_small = ERRV(DST_TOO_SMALL);
	S.err_mismatch = ERRV(SRC_SIZE_MISMATCH);
	S.err_too_large = ERRV(HDR_CMP_SIZE_TOO_LARGE);
	S.status = b->sizes;
	S.src = b->src;
	S.src_stride = b->src_stride;
	S.sample_bytes = J->sh.bytes;
	S.n = n;
	S.dst = b->dst;
	S.dst_stride = b->dst_stride;
	S.checksum = P->checksum_enabled ? 1u : 0u;
	for (c = 0; c < num_ctx; c++) {
		host_state[2u * c] = ctx[c].sequence_number;
		host_state[2u * c + 1u] = ctx[c].model_size;
	}
	e = airs_dev_h2d(dev, S.state, host_state, 8u * (size_t)num_ctx);
	if (!is_err(e))
		e = airs_dev_memset(dev, S.fb, 0, tb);
	if (!is_err(e) && work_buf_state(P)) {
		m = model_addressing(ctx, num_ctx);
		if (m.strided) {
			S.model = m.base;
			S.model_stride = m.stride;
		} else {
			m.base = NULL;
			S.model_ptrs = upload_model_ptrs(dev, ctx, J->ptrs, num_ctx);
			e = S.model_ptrs ? airs_dev_sync(dev) : ERRV(GENERIC);
		}
	}
	if (!is_err(e) && S.checksum)
		e = batch_checksums(J, &S.checksums);
	if (!is_err(e) && (b->flags & CMP_GPU_AUTO_RICE)) {
		d_g = airs_dev_scratch(dev, SLOT_G, (size_t)total * 4u);
		if (!d_g)
			e = ERRV(GENERIC);
	}
	for (a = 0; a <= fpc && !is_err(e); a++) {
		S.prev = (int32_t)a - 1;
		S.cur = a < fpc ? (int32_t)a : -1;
		e = airs_dev_fb_step(dev, &S);
		if (!is_err(e) && a > 0 && S.fb_eligible)
			e = airs_dev_fb_copy(dev, &S);
		if (a == fpc)
			break;
		for (uint32_t which = 0; which < (S.iters ? 2u : 1u) && !is_err(e); which++) {
			const struct pass *Q = which ? ps : pp;
			struct airs_launch L;

			launch_fill(&L, b, &J->sh, &ctx[0], Q, cap1);
			L.num_frames = num_ctx;
			L.frame_list = which ? S.flist_s : S.flist_p;
			if (d_g && pass_auto_rice(Q)) {
				L.auto_rice = 1;
				L.frame_g_scratch = d_g;
			}
			L.model = m.base;
			L.model_stride = m.stride;
			L.model_div = fpc;
			L.model_ptrs = S.model_ptrs;
			L.model_ptrs_al16 = m.al16;
			L.seqs = S.seqs; /* the device's state machine numbers the frames */
			L.seq = 0;
			L.checksums = S.checksums;
			e = airs_dev_encode(dev, &L);
		}
	}
	/* the one read-back: identifier draws and the final context states */
	if (!is_err(e))
		e = airs_dev_d2h(dev, host_draws, S.draws, total);
	if (!is_err(e))
		e = airs_dev_d2h(dev, host_state, S.state, 8u * (size_t)num_ctx);
	if (!is_err(e))
		e = airs_dev_sync(dev);
	if (is_err(e))
		goto out;
	draw_identifiers(ctx, num_ctx, fpc, host_draws, J->ids, REPORT_DRAWS(b) ? b->draws : NULL);
	for (c = 0; c < num_ctx; c++)
		ctx_commit(&ctx[c], J->ids[c * fpc + fpc - 1u], host_state[2u * c], host_state[2u * c + 1u]);
	e = commit_ids(J, COMMIT_SYNC, NULL);
out:
	free(host_state);
	return e;
}

/*
 * The three MODEL batch paths below hand the whole batch to airs_dev_walk
 * (enc_walk.hip): every frame, acquisition after acquisition, with each
 * context's model kept on the chip.  walk_prepare() decides what they share:
 * whether a walk applies at all, and the launch as far as the batch and the
 * contexts' parameters give it.
 */
struct walk_prep {
	struct airs_walk w;   /* the caller adds what is its own */
	uint32_t m_strided;   /* models at w.model + c * w.model_stride; else a pointer list (walk_upload) */
	uint32_t seq_same;    /* every context at ctx[0]'s sequence number (w.seq0) */
};

/* Returns 0 or WALK_NO; allocates and launches nothing.  A walk applies when
 * every context has the same parameters with a MODEL secondary pass and a
 * NONE/DIFF primary pass coded with the configured parameters, and the models
 * are strided or 16-byte aligned.  need_fb: the batch is in exact mode and the
 * uncompressed fallback must be the only way a frame's outcome can change the
 * next frame's pass: the fallback enabled with dst_capacity >= the raw frame
 * size (the first attempt's capacity is then the raw size, so a frame either
 * fits or falls back), and no secondary first frame whose model size differs
 * (no SRC_SIZE_MISMATCH). */
static uint32_t walk_prepare(const struct batch_job *J, int need_fb, struct walk_prep *pr)
{
	const struct cmp_context *ctx = J->ctx;
	const struct cmp_gpu_batch *b = J->b;
	const struct cmp_params *P = &ctx[0].params;
	const uint32_t num_ctx = J->num_ctx, n = J->sh.n, raw = raw_frame_size(&ctx[0], n);
	struct airs_walk *w = &pr->w;
	struct model_addr m;
	uint32_t c;

	if (!model_needed(P) || (P->primary_preprocessing != CMP_PREPROCESS_NONE &&
				 P->primary_preprocessing != CMP_PREPROCESS_DIFF))
		return WALK_NO;
	if (need_fb && (!fallback_applies(&ctx[0], b, n) || raw > 0xFFFFFFu))
		return WALK_NO;
	/* the walk codes with the configured parameters (AUTO_RICE: per-step launches) */
	if ((b->flags & CMP_GPU_AUTO_RICE) && P->primary_encoder_type == CMP_ENCODER_GOLOMB_ZERO)
		return WALK_NO;
	memset(pr, 0, sizeof(*pr));
	/* need_fb: the first attempt's capacity (cmp.c:358-366) */
	w->cap = need_fb ? raw : launch_cap(b->dst_capacity, n);
	pr->seq_same = 1;
	for (c = 0; c < num_ctx; c++) {
		const uint32_t sq = ctx[c].sequence_number;

		if (!same_params(&ctx[c].params, P))
			return WALK_NO;
		if (need_fb && sq != 0u && sq <= P->secondary_iterations && ctx[c].model_size != 2u * n)
			return WALK_NO; /* the reference returns SRC_SIZE_MISMATCH for that frame */
		if (sq != ctx[0].sequence_number)
			pr->seq_same = 0;
	}
	w->src = b->src;
	w->src_stride = b->src_stride;
	w->sample_bytes = J->sh.bytes;
	w->is_unsigned = J->sh.is_unsigned;
	w->n = n;
	w->num_ctx = num_ctx;
	w->fpc = J->fpc;
	w->dst = b->dst;
	w->dst_stride = b->dst_stride;
	w->pre_p = P->primary_preprocessing;
	w->enc_p = P->primary_encoder_type;
	w->g_p = P->primary_encoder_param;
	w->outl_p = P->primary_encoder_outlier;
	w->enc_s = P->secondary_encoder_type;
	w->g_s = P->secondary_encoder_param;
	w->outl_s = P->secondary_encoder_outlier;
	w->model_rate = P->model_rate;
	w->iters = P->secondary_iterations;
	w->checksum_enabled = P->checksum_enabled ? 1u : 0u;
	w->status = b->sizes;
	w->seq0 = ctx[0].sequence_number;
	/* model of context c: strided work buffers, or a list of aligned pointers */
	m = model_addressing(ctx, num_ctx);
	if (!m.strided && !m.al16)
		return WALK_NO;
	pr->m_strided = m.strided;
	w->model = m.base;
	w->model_stride = m.strided ? m.stride : 0;
	return 0;
}

/* can the device run the prepared walk?  Asked once the caller has set its
 * own fields; the pointer list is not uploaded yet (walk_prepare checked its
 * alignment), so it goes in without a model */
static int walk_supported(const struct walk_prep *pr)
{
	struct airs_walk chk = pr->w;

	if (!pr->m_strided)
		chk.model = NULL, chk.model_stride = 0;
	return airs_dev_walk_supported(&chk);
}

/* Device copies of what a walk cannot address by a rule: the work-buffer
 * pointers where the models are not strided, the identifiers where the caller
 * passes a list, and the contexts' first sequence numbers where they differ
 * (the byte at seq0 + c * step, into d_seq: device scratch of the caller's
 * choice).  One synchronise at the end; nothing is done for strided models at
 * one sequence number with affine identifiers. */
static uint32_t walk_upload(const struct batch_job *J, struct walk_prep *pr, const uint8_t *seq0, size_t step,
			    uint8_t *d_seq, const uint64_t *ids)
{
	struct airs_dev_engine *dev = J->dev;
	struct airs_walk *w = &pr->w;
	uint8_t *h_seq = NULL;
	uint32_t c, e = 0;

	if (pr->m_strided && pr->seq_same && !ids)
		return 0;
	if (!pr->m_strided) {
		w->model_ptrs = upload_model_ptrs(dev, J->ctx, J->ptrs, w->num_ctx);
		if (!w->model_ptrs)
			e = ERRV(GENERIC);
	}
	if (ids && !is_err(e)) {
		uint64_t *d_ids = airs_dev_scratch(dev, SLOT_IDS, (size_t)J->sh.total * 8u);

		e = d_ids ? airs_dev_h2d(dev, d_ids, ids, (size_t)J->sh.total * 8u) : ERRV(GENERIC);
		w->ids = d_ids;
	}
	if (!pr->seq_same && !is_err(e)) {
		h_seq = malloc(w->num_ctx);
		if (!h_seq || !d_seq)
			e = ERRV(GENERIC);
		for (c = 0; c < w->num_ctx && !is_err(e); c++)
			h_seq[c] = seq0[c * step];
		if (!is_err(e))
			e = airs_dev_h2d(dev, d_seq, h_seq, w->num_ctx);
		w->seq0s = d_seq;
	}
	if (!is_err(e))
		e = airs_dev_sync(dev);
	free(h_seq);
	return e;
}

/*
 * The walk in the asynchronous mode (no frame can fail or fall back): applies
 * when the plan the host replayed is the one the walk's pass rule gives.
 * Returns 0, an error value, or WALK_NO (not applicable; nothing launched).
 */
static uint32_t batch_walk(const struct batch_job *J)
{
	const struct frame_plan *plan = J->plan;
	const uint32_t num_ctx = J->num_ctx, fpc = J->fpc;
	struct walk_prep pr;
	struct airs_walk *w = &pr.w;
	uint32_t c, a, e, id_aff = 1;
	uint8_t *d_seq = NULL;

	if (walk_prepare(J, 0, &pr))
		return WALK_NO;
	/* the walk's pass rule (cmp.c:228-248), started from each context's
	 * first frame, must give the replayed plan frame by frame (the replay
	 * has advanced the contexts: the sequence numbers are the plan's) */
	pr.seq_same = 1;
	for (c = 0; c < num_ctx; c++) {
		uint32_t sq = plan[c * fpc].p.seq;

		if (sq != plan[0].p.seq)
			pr.seq_same = 0;
		for (a = 0; a < fpc; a++) {
			const struct pass *p = &plan[c * fpc + a].p;
			const int prim = sq == 0 || sq > w->iters;

			if (p->seq != (prim ? 0u : sq) ||
			    p->pre != (prim ? w->pre_p : (uint32_t)CMP_PREPROCESS_MODEL) ||
			    p->enc != (prim ? w->enc_p : w->enc_s) || p->par != (prim ? w->g_p : w->g_s) ||
			    p->model_mode != (prim ? (uint32_t)AIRS_MODEL_STORE : (uint32_t)AIRS_MODEL_UPDATE))
				return WALK_NO;
			sq = prim ? 1u : sq + 1u;
		}
	}
	w->seq0 = plan[0].p.seq;
	/* identifiers: base + c cstep + a astep, or a list */
	w->id_base = plan[0].id;
	w->id_cstep = num_ctx > 1 ? plan[fpc].id - plan[0].id : 0;
	w->id_astep = fpc > 1 ? plan[1].id - plan[0].id : 0;
	for (c = 0; c < num_ctx && id_aff; c++)
		for (a = 0; a < fpc && id_aff; a++)
			id_aff = plan[c * fpc + a].id == w->id_base + c * w->id_cstep + a * w->id_astep;
	if (!walk_supported(&pr))
		return WALK_NO;
	if (!id_aff)
		for (c = 0; c < J->sh.total; c++)
			J->ids[c] = plan[c].id;
	if (!pr.seq_same)
		d_seq = airs_dev_scratch(J->dev, SLOT_FL, num_ctx);
	e = walk_upload(J, &pr, &plan[0].p.seq, fpc * sizeof(*plan), d_seq, id_aff ? NULL : J->ids);
	if (!is_err(e) && w->checksum_enabled)
		e = batch_checksums(J, &w->checksums);
	return is_err(e) ? e : airs_dev_walk(J->dev, w);
}

/*
 * MODEL contexts with the uncompressed fallback in one launch (the context
 * walk, enc_walk.hip): the walk resolves each frame's fallback on the chip
 * (cmp.c:342-393) and reports every frame's identifier draws and each
 * context's final sequence number; one read-back, then the identifiers are
 * drawn in call order and patched into the headers, as batch_device_exact
 * does.  Returns 0, an error value, or WALK_NO.
 */
static uint32_t batch_walk_fb(const struct batch_job *J)
{
	struct airs_dev_engine *dev = J->dev;
	struct cmp_context *ctx = J->ctx;
	const uint32_t num_ctx = J->num_ctx, fpc = J->fpc, total = J->sh.total;
	const size_t tb = ((size_t)total + 15u) & ~(size_t)15u;
	/* page-locked host scratch: draws [tb], final sequence numbers [num_ctx]
	 * (one read-back of the device scratch's first tb + num_ctx bytes), then
	 * the identifiers [total] at the next 8-byte boundary */
	const size_t ioff = (tb + num_ctx + 7u) & ~(size_t)7u;
	struct walk_prep pr;
	struct airs_walk *w = &pr.w;
	uint32_t c, e;
	uint8_t *scr, *h_draws;

	if (walk_prepare(J, 1, &pr))
		return WALK_NO;
	w->fb = 1;
	w->raw_size = w->cap;
	/* scratch: draws [tb], final sequence numbers [num_ctx], first sequence
	 * numbers [num_ctx]; requested before the device is asked, which wants
	 * to see draws and seq_out */
	scr = airs_dev_scratch(dev, SLOT_FL, tb + 2u * (size_t)num_ctx + 16u);
	if (!scr)
		return ERRV(GENERIC);
	w->draws = scr;
	w->seq_out = scr + tb;
	if (!walk_supported(&pr))
		return WALK_NO;
	h_draws = airs_dev_host_scratch(dev, ioff + (size_t)total * 8u);
	if (!h_draws)
		return ERRV(GENERIC);
	e = walk_upload(J, &pr, &ctx[0].sequence_number, sizeof(*ctx), scr + tb + num_ctx, NULL);
	if (!is_err(e) && w->checksum_enabled)
		e = batch_checksums(J, &w->checksums);
	if (!is_err(e))
		e = airs_dev_walk(dev, w);
	/* the one read-back: identifier draws and the final sequence numbers
	 * (adjacent in the device scratch, one copy into page-locked memory) */
	if (!is_err(e))
		e = airs_dev_d2h(dev, h_draws, w->draws, tb + num_ctx);
	if (!is_err(e))
		e = airs_dev_sync(dev);
	if (is_err(e))
		return e;
	/* the identifiers first; the contexts advance only once the headers are
	 * patched (a failed upload or patch leaves them as they were) */
	draw_identifiers(ctx, num_ctx, fpc, h_draws, J->ids, NULL);
	/* upload from page-locked memory and patch, both asynchronous
	 * (cmp_gpu_synchronize waits; the next call rewrites the host scratch
	 * only after its own read-back, which follows them) */
	e = commit_ids(J, COMMIT_ASYNC, (uint64_t *)(void *)(h_draws + ioff));
	if (is_err(e))
		return e;
	if (REPORT_DRAWS(J->b))
		memcpy(J->b->draws, h_draws, total);
	for (c = 0; c < num_ctx; c++) /* every context's model holds a frame of this size */
		ctx_commit(&ctx[c], J->ids[c * fpc + fpc - 1u], h_draws[tb + c], 2u * J->sh.n);
	return e;
}

/*
 * MODEL contexts with the uncompressed fallback where the context walk does
 * not apply (frames of another size, or too few contexts to fill the CUs):
 * the segment walk codes every frame as if none fell back, with the raw frame
 * size as the capacity, so a frame that would fall back reports DST_TOO_SMALL
 * (the reference's first attempt, cmp.c:358-366) and nothing else changes for
 * the frames that fit.  One read-back of the statuses; a context with such a
 * frame (data that does not compress: rare) gets its model back from a copy
 * taken before the launch and runs again on the per-acquisition device state
 * machine (batch_device_exact), in call order, so the identifiers are drawn as
 * the call loop draws them.  The other contexts' identifiers follow the pass
 * rule (one draw per primary pass) and are patched into their headers.
 * Returns 0, an error value, or WALK_NO.
 */
static uint32_t batch_walk_spec(const struct batch_job *J, const struct pass *pp, const struct pass *ps)
{
	struct airs_dev_engine *dev = J->dev;
	struct cmp_context *ctx = J->ctx;
	const struct cmp_gpu_batch *b = J->b;
	const uint32_t num_ctx = J->num_ctx, fpc = J->fpc, total = J->sh.total;
	const size_t mb = 2u * (size_t)J->sh.n; /* model bytes of a context */
	struct walk_prep pr;
	struct airs_walk *w = &pr.w;
	uint32_t c, a, e, msec = 0, cseq = 0, any_redo = 0;
	uint8_t *msave, *redo, *d_seq = NULL;
	uint64_t *h_ids;

	if (num_ctx > AIRS_COMMIT_MAX_CTX || walk_prepare(J, 1, &pr))
		return WALK_NO;
	if (!walk_supported(&pr)) /* identifiers 0: patched once they are drawn */
		return WALK_NO;
	/* page-locked host scratch: the identifiers for patch_ids_kernel (when
	 * the commit kernel does not take them) */
	msave = airs_dev_scratch(dev, SLOT_MSAVE, mb * num_ctx);
	h_ids = airs_dev_host_scratch(dev, (size_t)total * 8u);
	redo = calloc(num_ctx, 1);
	if (!msave || !h_ids || !redo) {
		e = ERRV(GENERIC);
		goto out;
	}
	if (!pr.seq_same)
		d_seq = airs_dev_scratch(dev, SLOT_FL, num_ctx);
	e = walk_upload(J, &pr, &ctx[0].sequence_number, sizeof(*ctx), d_seq, NULL);
	/* the models as they are before the launch, for contexts run again whose
	 * first frame reads its model (a secondary pass; a primary pass stores
	 * the model without reading it) */
	for (c = 0; c < num_ctx; c++)
		if (ctx[c].sequence_number != 0u && ctx[c].sequence_number <= w->iters)
			msec = 1;
	if (!is_err(e) && msec) {
		if (pr.m_strided)
			e = airs_dev_d2d_rows(dev, msave, mb, ctx[0].work_buf, num_ctx > 1 ? w->model_stride : mb, mb,
					      num_ctx);
		else
			for (c = 0; c < num_ctx && !is_err(e); c++)
				e = airs_dev_d2d_rows(dev, msave + c * mb, mb, ctx[c].work_buf, mb, mb, 1);
	}
	if (!is_err(e) && w->checksum_enabled)
		e = batch_checksums(J, &w->checksums);
	/* the one round trip: which contexts have a frame that did not fit.  The
	 * commit kernel signals them, then waits on the stream for the release
	 * below (it patches the identifiers when no context runs again) */
	if (!is_err(e))
		e = airs_dev_walk(dev, w);
	if (!is_err(e)) {
		e = airs_dev_commit_begin(dev, b->sizes, num_ctx, fpc, b->dst, b->dst_stride, &cseq);
		if (!is_err(e)) {
			e = airs_dev_commit_wait(dev, cseq, num_ctx, redo);
			for (c = 0; c < num_ctx && !is_err(e) && !any_redo; c++)
				any_redo = redo[c];
			if (is_err(e) || any_redo) {
				(void)airs_dev_commit_release(dev, cseq, NULL, 0);
				if (is_err(e)) {
					(void)airs_dev_sync(dev); /* reports and clears the fault count */
					goto out;
				}
			}
		}
	}
	if (is_err(e))
		goto out;
	/* in call order: the pass rule's draws, or the context run again */
	for (c = 0; c < num_ctx && !is_err(e); c++) {
		if (!redo[c]) {
			uint32_t sq = ctx[c].sequence_number;
			uint64_t id = ctx[c].identifier;

			for (a = 0; a < fpc; a++) {
				const int prim = sq == 0u || sq > w->iters;

				if (prim)
					id = next_identifier();
				J->ids[c * fpc + a] = id;
				if (REPORT_DRAWS(b))
					b->draws[c * fpc + a] = prim ? 1u : 0u;
				sq = prim ? 1u : sq + 1u;
			}
		} else {
			/* the context's frames as a batch of their own */
			struct cmp_gpu_batch sb = *b;
			struct batch_job sub = *J;

			if (msec)
				e = airs_dev_d2d_rows(dev, ctx[c].work_buf, mb, msave + c * mb, mb, mb, 1);
			sb.src = (const uint8_t *)b->src + (uint64_t)c * fpc * b->src_stride;
			sb.dst = (uint8_t *)b->dst + (uint64_t)c * fpc * b->dst_stride;
			sb.sizes = b->sizes + (size_t)c * fpc;
			sb.draws = b->draws ? b->draws + (size_t)c * fpc : NULL;
			sub.b = &sb;
			sub.ctx = &ctx[c];
			sub.num_ctx = 1;
			sub.sh.total = fpc;
			sub.ids = J->ids + (size_t)c * fpc;
			if (!is_err(e))
				e = batch_device_exact(&sub, pp, ps);
		}
	}
	if (is_err(e))
		goto out;
	/* the identifiers: released to the waiting commit kernel, or (a context
	 * ran again, or more frames than its block holds) patched by
	 * patch_ids_kernel from page-locked memory (batch_device_exact does not
	 * use the host scratch) */
	if (any_redo || !airs_dev_commit_release(dev, cseq, J->ids, total)) {
		e = commit_ids(J, COMMIT_DIRECT, h_ids);
		if (is_err(e))
			goto out;
	}
	for (c = 0; c < num_ctx; c++) {
		uint32_t sq = ctx[c].sequence_number;

		if (redo[c])
			continue; /* committed by batch_device_exact */
		for (a = 0; a < fpc; a++) /* the pass rule again */
			sq = sq == 0u || sq > w->iters ? 1u : sq + 1u;
		ctx_commit(&ctx[c], J->ids[c * fpc + fpc - 1u], sq, 2u * J->sh.n);
	}
out:
	free(redo);
	return e;
}

/*
 * IWT contexts without a MODEL pass, every frame of the batch on the same
 * pass (asynchronous mode): all frames in ONE launch instead of one per
 * acquisition.  The reference computes a frame's coefficients into its
 * context's work buffer (preprocess.c:321-353), so after the batch that
 * buffer holds the coefficients of the context's last frame; the other
 * frames' coefficients go to device scratch (at most IWT_SCRATCH_MAX bytes,
 * else WALK_NO: the per-acquisition launches).
 */
static uint32_t batch_iwt(const struct batch_job *J)
{
	const uint32_t num_ctx = J->num_ctx, fpc = J->fpc, total = J->sh.total;
	const uint64_t cstride = (2ull * J->sh.n + 15u) & ~15ull;
	const uint64_t need = (uint64_t)(total - num_ctx) * cstride;
	uint64_t k = 0;
	uint8_t *scr;
	uint32_t c, a, e;

	if (fpc < 2 || need > IWT_SCRATCH_MAX)
		return WALK_NO;
	scr = airs_dev_scratch(J->dev, SLOT_MODEL, (size_t)need);
	if (!scr)
		return WALK_NO;
	for (c = 0; c < num_ctx; c++)
		for (a = 0; a < fpc; a++)
			J->ptrs[c * fpc + a] = a + 1u == fpc ? (uint64_t)(uintptr_t)J->ctx[c].work_buf
							     : (uint64_t)(uintptr_t)(scr + (k++) * cstride);
	e = batch_launch(J, NULL, 0, 1, total, J->b->dst_capacity, 1);
	return e == WALK_NO ? ERRV(GENERIC) : e;
}

uint32_t cmp_gpu_compress(struct cmp_gpu_engine *eng, struct cmp_context *ctx, uint32_t num_ctx,
			  uint32_t fpc, const struct cmp_gpu_batch *b)
{
	return cmp_batch_compress(eng, ctx, num_ctx, fpc, b);
}

uint32_t cmp_context_usable(const struct cmp_context *ctx)
{
	if (ctx->magic != CTX_MAGIC)
		return ERRV(CONTEXT_INVALID);
	if (work_buf_state(&ctx->params) && ((uintptr_t)ctx->work_buf & 1u))
		return ERRV(WORK_BUF_UNALIGNED);
	return 0;
}

/* what the call refuses before it plans anything; fills in the shape */
static uint32_t batch_validate(const struct cmp_gpu_engine *eng, const struct cmp_context *ctx, uint32_t num_ctx,
			       uint32_t fpc, const struct cmp_gpu_batch *b, struct batch_shape *sh)
{
	const uint32_t bytes = b && b->type == CMP_GPU_I16_IN_I32 ? 4u : 2u;
	uint32_t c, e;

	if (!eng || !ctx || !b || !num_ctx || !fpc)
		return ERRV(GENERIC);
	if (b->type > CMP_GPU_I16_IN_I32)
		return ERRV(PARAMS_INVALID);
	if (!b->src)
		return ERRV(SRC_NULL);
	if (b->src_size == 0 || b->src_size % bytes)
		return ERRV(SRC_SIZE_WRONG);
	if (((uintptr_t)b->src % bytes) || (b->src_stride % bytes)) {
		fprintf(stderr, "airscmp: cmp_gpu_compress: src must be %u-byte aligned\n", bytes);
		return ERRV(GENERIC);
	}
	if (!b->sizes) {
		fprintf(stderr, "airscmp: cmp_gpu_compress: sizes array is NULL\n");
		return ERRV(GENERIC);
	}
	if ((b->flags & CMP_GPU_REPORT_DRAWS) && !b->draws) {
		fprintf(stderr, "airscmp: cmp_gpu_compress: CMP_GPU_REPORT_DRAWS without a draws array\n");
		return ERRV(GENERIC);
	}
	if (b->draws && !(b->flags & CMP_GPU_REPORT_DRAWS)) {
		/* callers of the earlier interface set draws alone: it is left
		 * untouched now, say so once */
		static int warned;
		if (!warned) {
			warned = 1;
			fprintf(stderr, "airscmp: cmp_gpu_compress: draws array given without CMP_GPU_REPORT_DRAWS: "
					"not written\n");
		}
	}
	if (!b->dst)
		return ERRV(DST_NULL);
	if (((uintptr_t)b->dst & 7u) || (b->dst_stride & 7u))
		return ERRV(DST_UNALIGNED);
	if (is_err(b->dst_capacity))
		return ERRV(GENERIC);
	if ((uint64_t)num_ctx * fpc > 0xFFFFFFFull)
		return ERRV(PARAMS_INVALID);
	*sh = (struct batch_shape){ bytes, b->src_size / bytes, num_ctx * fpc, b->type == CMP_GPU_U16 };
	/* frames of a batch must not overlap: every workgroup of a frame writes
	 * up to min(capacity, worst-case frame) bytes from its frame base */
	if (sh->total > 1) {
		const uint64_t span = launch_cap(b->dst_capacity, sh->n);

		if (b->src_stride < b->src_size || b->dst_stride < span) {
			fprintf(stderr, "airscmp: cmp_gpu_compress: frames overlap (src_stride %llu < src_size %u "
					"or dst_stride %llu < %llu)\n",
				(unsigned long long)b->src_stride, b->src_size, (unsigned long long)b->dst_stride,
				(unsigned long long)span);
			return ERRV(GENERIC);
		}
	}
	for (c = 0; c < num_ctx; c++)
		if (is_err(e = cmp_context_usable(&ctx[c])))
			return e;
	return 0;
}

/* Must the batch run step by step (exact mode)?  Yes where a context's
 * frames can fall back to raw storage.  And a frame that can fail changes its context's next pass (the reference
 * does not advance sequence_number on an error), so such batches run step
 * by step: capacity below the worst case, or a worst case past the 24-bit
 * size field (n > ~2.8 Mi samples: HDR_CMP_SIZE_TOO_LARGE is possible)
 * when a context has secondary passes.  Without secondary passes every
 * frame is a primary pass with one identifier draw whatever the outcome
 * of the frame before, so the plan does not depend on it; the context's
 * sequence number after the call still does (a context whose last frame
 * fails stays at 0, cmp.c:321-338, and with secondary passes the next
 * call's first pass follows from it), so a batch whose coder can take a
 * frame past the size field runs step by step as well.  A coder whose
 * longest codeword keeps every frame within the field (cfg2's g = 32 at
 * 4 Mi samples: 22 bits per sample) cannot fail and stays asynchronous. */
static int batch_must_step(const struct batch_job *J)
{
	const struct cmp_gpu_batch *b = J->b;
	const uint32_t n = J->sh.n;
	const int past_field = is_err(cmp_compress_bound(2u * n));
	uint32_t c;

	if ((uint64_t)b->dst_capacity < HDR_MAX_SIZE + CMP_CHECKSUM_SIZE + payload_bound(2u * n))
		return 1;
	for (c = 0; c < J->num_ctx; c++) {
		const struct cmp_params *P = &J->ctx[c].params;

		if (fallback_applies(&J->ctx[c], b, n))
			return 1;
		if (past_field && ((P->secondary_iterations && J->fpc > 1) || size_field_can_overflow(P, n, b->flags)))
			return 1;
	}
	return 0;
}

/* The plan of the asynchronous mode: replay the context state machine in call
 * order (c-major), counting identifier draws, then draw the identifiers.  A
 * frame the host API would reject sends the batch to the step-by-step path
 * with the contexts untouched (*exact).  Returns 0 or an error value. */
static uint32_t batch_replay(const struct batch_job *J, int *exact)
{
	struct cmp_context *ctx = J->ctx;
	const struct cmp_gpu_batch *b = J->b;
	const uint32_t num_ctx = J->num_ctx, fpc = J->fpc;
	/* the contexts as they came, then the draws of every frame */
	struct cmp_context *snap = calloc(1, (size_t)num_ctx * sizeof(*snap) + J->sh.total);
	uint8_t *draws = (uint8_t *)(snap + num_ctx);
	uint32_t c, a;

	if (!snap)
		return ERRV(GENERIC);
	memcpy(snap, ctx, (size_t)num_ctx * sizeof(*snap));
	for (c = 0; c < num_ctx && !*exact; c++) {
		for (a = 0; a < fpc; a++) {
			const uint32_t f = c * fpc + a;
			void *dst = (uint8_t *)b->dst + (uint64_t)f * b->dst_stride;
			uint32_t drawn = 0;

			if (is_err(engine_prologue(&ctx[c], dst, b->dst_capacity, J->sh.n, &J->plan[f].p, &drawn))) {
				*exact = 1;
				break;
			}
			draws[f] = (uint8_t)drawn;
			ctx[c].sequence_number++;
		}
	}
	if (*exact) {
		memcpy(ctx, snap, (size_t)num_ctx * sizeof(*snap));
	} else {
		/* the identifiers, drawn in call order (the replay's resets
		 * cleared the contexts': they start from the snapshot's) */
		draw_identifiers(snap, num_ctx, fpc, draws, J->ids, REPORT_DRAWS(b) ? b->draws : NULL);
		for (c = 0; c < num_ctx; c++) {
			for (a = 0; a < fpc; a++)
				J->plan[c * fpc + a].id = J->ids[c * fpc + a];
			ctx[c].identifier = J->ids[c * fpc + fpc - 1u];
		}
	}
	free(snap);
	return 0;
}

/* exact mode's routes */
static uint32_t dispatch_exact(const struct batch_job *J)
{
	const uint32_t flags = J->b->flags;
	struct pass pp, ps;
	uint32_t e;

	/* contexts that differ, or a frame the prologue rejects: step on the host */
	if ((flags & CMP_GPU_HOST_STEPPED) || !device_exact_ok(J, &pp, &ps))
		return batch_exact(J);
	/* MODEL contexts with the fallback: every acquisition in one launch (or an error) */
	if (!(flags & CMP_GPU_STEPWISE) &&
	    ((e = batch_walk_fb(J)) != WALK_NO || (e = batch_walk_spec(J, &pp, &ps)) != WALK_NO))
		return e;
	return batch_device_exact(J, &pp, &ps);
}

/* asynchronous mode's routes: frames with equal passes
 * share one launch; contexts with state in their work buffers (the model, IWT
 * coefficients) take their acquisitions in order */
static uint32_t dispatch_async(const struct batch_job *J)
{
	const struct frame_plan *plan = J->plan;
	const uint32_t num_ctx = J->num_ctx, fpc = J->fpc, total = J->sh.total, cap = J->b->dst_capacity;
	const int stepwise = (J->b->flags & CMP_GPU_STEPWISE) != 0;
	uint32_t a, c, f, g, e = 0, any_model = 0, any_mneed = 0, uniform = 1;
	struct step_scratch s;

	for (c = 0; c < num_ctx; c++) {
		any_mneed |= model_needed(&J->ctx[c].params) != 0;
		any_model |= work_buf_state(&J->ctx[c].params) != 0;
	}
	for (f = 1; f < total && uniform; f++)
		uniform = same_pass(&plan[f].p, &plan[0].p);
	if (!any_model && (num_ctx == 1 || fpc == 1 || uniform)) {
		/* contiguous runs of frames with the same pass, one launch each */
		for (f = 0; f < total && !is_err(e); f = g) {
			g = f + 1;
			while (g < total && same_pass(&plan[g].p, &plan[f].p))
				g++;
			e = batch_launch(J, NULL, f, 1, g - f, cap, 0);
		}
		return e;
	}
	if (uniform && !any_mneed && plan[0].p.pre == CMP_PREPROCESS_IWT && !stepwise && (e = batch_iwt(J)) != WALK_NO)
		return e; /* IWT contexts: every frame in one launch (or an error) */
	if (any_model && !stepwise && (e = batch_walk(J)) != WALK_NO)
		return e; /* every acquisition in one launch (or an error) */
	/* one launch per acquisition step across the contexts (one per pass when
	 * contexts are in different states); MODEL contexts carry state from one
	 * step to the next */
	if (!step_scratch_alloc(&s, num_ctx, 0))
		return ERRV(GENERIC);
	for (a = 0, e = 0; a < fpc && !is_err(e); a++) {
		for (c = 0; c < num_ctx; c++) {
			s.list[c] = c * fpc + a;
			s.caps[c] = cap;
		}
		e = launch_groups(J, &s, num_ctx);
	}
	free(s.id0);
	return e;
}

uint32_t cmp_batch_compress(struct cmp_gpu_engine *eng, struct cmp_context *ctx, uint32_t num_ctx, uint32_t fpc,
			    const struct cmp_gpu_batch *b)
{
	struct batch_job J;
	int exact;
	uint32_t e = batch_validate(eng, ctx, num_ctx, fpc, b, &J.sh);

	if (is_err(e))
		return e;
	/* one allocation: the plan, then the identifiers, then the pointer staging */
	J = (struct batch_job){ eng->dev, ctx, num_ctx, fpc, b, J.sh, calloc(J.sh.total, sizeof(*J.plan) + 16u), NULL, NULL };
	if (!J.plan)
		return ERRV(GENERIC);
	J.ids = (uint64_t *)(J.plan + J.sh.total);
	J.ptrs = J.ids + J.sh.total;
	exact = batch_must_step(&J);
	if (!exact)
		e = batch_replay(&J, &exact);
	if (!is_err(e))
		e = exact ? dispatch_exact(&J) : dispatch_async(&J);
	free(J.plan);
	return is_err(e) ? e : 0;
}
