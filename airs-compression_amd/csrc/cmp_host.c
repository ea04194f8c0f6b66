/*
 * cmp_host.c -- host side of libairscmp.so: the cmp.h API (drop-in for the
 * reference's lib/compress/cmp.c + lib/common/cmp_errors.c) and the thin
 * cmp_gpu.h wrappers; the batch planner behind cmp_gpu_compress is
 * cmp_batch.c, which shares cmp_pass.h with this file.  Parameter validation,
 * the context state machine (primary/secondary passes, identifiers, fallback)
 * and all error codes follow the reference exactly; the per-sample work is
 * done by the HIP kernels in encode.hip through airs_dev.h.  There is no CPU
 * encode path: without a usable GPU the compress calls fail with
 * CMP_ERR_GENERIC and a message on stderr.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cmp_engine.h"
#include "cmp_pass.h"

#define MAX_MODEL_RATE 16u

/* ---------------- identifiers (reference cmp.c:27-50, 438-449) ---------------- */
static uint64_t g_counter;

static void counter_timestamp(uint32_t *coarse, uint16_t *fine)
{
	*coarse = (uint32_t)(g_counter >> 16);
	*fine = (uint16_t)g_counter;
	g_counter++;
}

static void (*g_timestamp)(uint32_t *, uint16_t *) = counter_timestamp;

void cmp_set_timestamp_func(void (*f)(uint32_t *coarse, uint16_t *fine))
{
	g_timestamp = f ? f : counter_timestamp;
}

uint64_t next_identifier(void)
{
	uint32_t coarse = 0;
	uint16_t fine = 0;

	g_timestamp(&coarse, &fine);
	return ((uint64_t)coarse << 16) | (uint64_t)fine;
}

/* ---------------- errors (reference lib/common/cmp_errors.c) ---------------- */
unsigned int cmp_is_error(uint32_t code)
{
	return is_err(code);
}

enum cmp_error cmp_get_error_code(uint32_t code)
{
	if (!is_err(code))
		return CMP_ERR_NO_ERROR;
	return (enum cmp_error)(0u - code);
}

const char *cmp_get_error_string(enum cmp_error code)
{
	static const struct {
		enum cmp_error code;
		const char *text;
	} table[] = {
		{ CMP_ERR_NO_ERROR, "No error detected" },
		{ CMP_ERR_GENERIC, "Error (generic)" },
		{ CMP_ERR_PARAMS_INVALID, "Invalid compression parameters" },
		{ CMP_ERR_DST_TOO_SMALL, "Destination buffer is too small to hold the content" },
		{ CMP_ERR_DST_NULL, "Destination buffer pointer is NULL" },
		{ CMP_ERR_DST_UNALIGNED, "Destination buffer pointer is unaligned" },
		{ CMP_ERR_SRC_SIZE_WRONG, "Source buffer size is invalid" },
		{ CMP_ERR_SRC_NULL, "Source buffer pointer is NULL" },
		{ CMP_ERR_SRC_SIZE_MISMATCH,
		  "Source data size changed using model preprocessing; not allowed until reset" },
		{ CMP_ERR_WORK_BUF_TOO_SMALL, "Work buffer is too small" },
		{ CMP_ERR_WORK_BUF_NULL, "Work buffer is NULL but required" },
		{ CMP_ERR_WORK_BUF_UNALIGNED, "Work buffer is unaligned" },
		{ CMP_ERR_HDR_CMP_SIZE_TOO_LARGE, "Compressed size exceeds header field limit" },
		{ CMP_ERR_HDR_ORIGINAL_TOO_LARGE, "Original size exceeds header field limit" },
		{ CMP_ERR_CONTEXT_INVALID, "Compression context uninitialised or corrupted" },
		{ CMP_ERR_INT_HDR, "Internal header processing error" },
		{ CMP_ERR_INT_ENCODER, "Internal data encoder error" },
		{ CMP_ERR_INT_BITSTREAM, "Internal bitstream writer error" },
	};
	size_t i;

	for (i = 0; i < sizeof(table) / sizeof(table[0]); i++)
		if (table[i].code == code)
			return table[i].text;
	return "Unspecified error code";
}

const char *cmp_get_error_message(uint32_t code)
{
	return cmp_get_error_string(cmp_get_error_code(code));
}

/* ---------------- encoder parameters (reference encoder.c:63-233) ---------------- */
static uint32_t floor_log2(uint32_t x)
{
	return 31u - (uint32_t)__builtin_clz(x);
}

/* validate (type, g, outlier) and resolve the outlier written to the header
 * (declared in cmp_engine.h: cmp_decode_stream.c resolves a stream's encoder
 * arguments with it) */
uint32_t cmp_coder_resolve(uint32_t type, uint32_t g, uint32_t outlier, uint32_t *resolved)
{
	uint32_t k, cutoff, limit;
	uint64_t want;

	if (resolved)
		*resolved = 0;
	if (type == CMP_ENCODER_UNCOMPRESSED)
		return 0;
	if (type != CMP_ENCODER_GOLOMB_ZERO && type != CMP_ENCODER_GOLOMB_MULTI)
		return ERRV(PARAMS_INVALID);
	if (g < 1u || g > 0xFFFFu)
		return ERRV(PARAMS_INVALID);
	k = floor_log2(g);
	cutoff = (2u << k) - g;
	limit = cutoff + (31u - k) * g; /* first value needing a > 32-bit codeword */
	if (type == CMP_ENCODER_GOLOMB_MULTI)
		limit = limit > 8u ? limit - 8u : 0u; /* 8 escape symbols for 16-bit samples */
	want = type == CMP_ENCODER_GOLOMB_ZERO ? (uint64_t)cutoff + 16ull * g - 1ull : (uint64_t)outlier;
	if (want > limit)
		want = limit;
	if (want == 0)
		return ERRV(PARAMS_INVALID);
	if (resolved)
		*resolved = (uint32_t)want;
	return 0;
}

/* 48 bits per sample worst case (reference encoder.c:381-386) */
uint64_t payload_bound(uint32_t size)
{
	uint64_t n = ((uint64_t)size * 8u + 15u) / 16u;

	return (n * 48u + 7u) / 8u;
}

uint32_t cmp_compress_bound(uint32_t packed_size)
{
	uint64_t b;

	if (packed_size > CMP_HDR_MAX_ORIGINAL_SIZE)
		return ERRV(HDR_ORIGINAL_TOO_LARGE);
	b = HDR_MAX_SIZE + CMP_CHECKSUM_SIZE + payload_bound(packed_size);
	if (b > CMP_HDR_MAX_COMPRESSED_SIZE)
		return ERRV(HDR_CMP_SIZE_TOO_LARGE);
	return (uint32_t)b;
}

static uint32_t pre_work_size(uint32_t pre, uint32_t size, int *known)
{
	*known = 1;
	if (pre == CMP_PREPROCESS_NONE || pre == CMP_PREPROCESS_DIFF)
		return 0;
	if (pre == CMP_PREPROCESS_IWT || pre == CMP_PREPROCESS_MODEL)
		return (size + 1u) & ~1u;
	*known = 0;
	return 0;
}

uint32_t cmp_cal_work_buf_size(const struct cmp_params *params, uint32_t src_size)
{
	uint32_t a, b = 0;
	int known;

	if (!params)
		return ERRV(GENERIC);
	if (params->primary_preprocessing == CMP_PREPROCESS_MODEL)
		return ERRV(PARAMS_INVALID);
	a = pre_work_size(params->primary_preprocessing, src_size, &known);
	if (!known)
		return ERRV(PARAMS_INVALID);
	if (params->secondary_iterations) {
		b = pre_work_size(params->secondary_preprocessing, src_size, &known);
		if (!known)
			return ERRV(PARAMS_INVALID);
	}
	return a > b ? a : b;
}

int model_needed(const struct cmp_params *p)
{
	return p->secondary_preprocessing == CMP_PREPROCESS_MODEL && p->secondary_iterations != 0;
}

/* some pass of the context keeps state in its work buffer: the model, or the
 * IWT coefficients (preprocess.c:321-353 computes them into work_buf), so
 * frames of one context cannot share a launch */
int work_buf_state(const struct cmp_params *p)
{
	return model_needed(p) || p->primary_preprocessing == CMP_PREPROCESS_IWT ||
	       (p->secondary_iterations && p->secondary_preprocessing == CMP_PREPROCESS_IWT);
}

/* cmp_reset; with `draws` set the identifier draw is only counted (the batch
 * API draws the identifiers afterwards, in the reference's call order) */
uint32_t ctx_reset(struct cmp_context *ctx, uint32_t *draws)
{
	if (!ctx)
		return ERRV(GENERIC);
	if (ctx->magic != CTX_MAGIC)
		return ERRV(CONTEXT_INVALID);
	ctx->sequence_number = 0;
	if (draws) {
		(*draws)++;
		ctx->identifier = 0;
	} else {
		ctx->identifier = next_identifier();
	}
	ctx->model_size = 0;
	return ERRV(NO_ERROR);
}

uint32_t cmp_reset(struct cmp_context *ctx)
{
	return ctx_reset(ctx, NULL);
}

void cmp_deinitialise(struct cmp_context *ctx)
{
	if (ctx)
		memset(ctx, 0, sizeof(*ctx));
}

uint32_t cmp_initialise(struct cmp_context *ctx, const struct cmp_params *params, void *work_buf,
			uint32_t work_buf_size)
{
	uint32_t e, need;

	if (!ctx)
		return ERRV(GENERIC);
	cmp_deinitialise(ctx);
	if (!params || is_err(work_buf_size))
		return ERRV(GENERIC);
	if (params->secondary_iterations >= (1u << CMP_HDR_BITS_SEQUENCE_NUMBER))
		return ERRV(PARAMS_INVALID);
	e = cmp_coder_resolve(params->primary_encoder_type, params->primary_encoder_param,
			  params->primary_encoder_outlier, NULL);
	if (is_err(e))
		return e;
	if (params->secondary_iterations) {
		e = cmp_coder_resolve(params->secondary_encoder_type, params->secondary_encoder_param,
				  params->secondary_encoder_outlier, NULL);
		if (is_err(e))
			return e;
	}
	if (model_needed(params) && params->model_rate > MAX_MODEL_RATE)
		return ERRV(PARAMS_INVALID);
	need = cmp_cal_work_buf_size(params, 2);
	if (is_err(need))
		return need;
	if (need) {
		if (!work_buf)
			return ERRV(WORK_BUF_NULL);
		if (!work_buf_size)
			return ERRV(WORK_BUF_TOO_SMALL);
		if ((uintptr_t)work_buf & 1u)
			return ERRV(WORK_BUF_UNALIGNED);
	}
	ctx->params = *params;
	ctx->work_buf = work_buf;
	ctx->work_buf_size = work_buf_size;
	ctx->magic = CTX_MAGIC;
	return cmp_reset(ctx);
}

/* ================================================================== */
/* one frame through the GPU (reference compress_engine, cmp.c:213-338) */
/* ================================================================== */
enum sample_kind { KIND_I16 = 0, KIND_I16_IN_I32 = 1, KIND_U16 = 2 };

struct frame_io {
	const void *src;   /* host or device, see `device` */
	uint32_t n;        /* samples */
	uint32_t bytes;    /* 2 or 4 per sample */
	enum sample_kind kind;
	int device;        /* src/dst/work_buf are device pointers (cmp_gpu.h path) */
	struct airs_dev_engine *dev;
	/* device-mode extras */
	uint32_t *d_status;
};

/* The host-pointer API stages every frame through one process-wide engine
 * (device scratch slots, look-back state).  Calls on different contexts may
 * come from different threads (the reference allows one context per thread),
 * so host_compress() holds g_host_lock for the whole call: calls are
 * serialised, and the engine is created once, under the lock. */
static pthread_mutex_t g_host_lock = PTHREAD_MUTEX_INITIALIZER;
static struct airs_dev_engine *g_host_dev;

static struct airs_dev_engine *host_dev(void)
{
	if (!g_host_dev) {
		g_host_dev = airs_dev_engine_create(NULL);
		if (!g_host_dev)
			fprintf(stderr, "airscmp: no usable GPU (%s); libairscmp has no CPU encode path\n",
				airs_dev_last_error());
	}
	return g_host_dev;
}

/* checks and state updates of compress_engine up to the encode loop;
 * returns 0 (pass filled in) or the error the reference would return */
uint32_t engine_prologue(struct cmp_context *ctx, void *dst, uint32_t cap, uint32_t n, struct pass *p,
			 uint32_t *draws)
{
	const uint32_t packed = 2u * n;
	uint32_t e;

	memset(p, 0, sizeof(*p));
	if (ctx->sequence_number == 0 || ctx->sequence_number > ctx->params.secondary_iterations) {
		e = ctx_reset(ctx, draws);
		if (is_err(e))
			return e;
		p->pre = ctx->params.primary_preprocessing;
		p->enc = ctx->params.primary_encoder_type;
		p->par = ctx->params.primary_encoder_param;
		p->outlier_param = ctx->params.primary_encoder_outlier;
		ctx->model_size = packed;
	} else {
		p->pre = ctx->params.secondary_preprocessing;
		p->enc = ctx->params.secondary_encoder_type;
		p->par = ctx->params.secondary_encoder_param;
		p->outlier_param = ctx->params.secondary_encoder_outlier;
		if (model_needed(&ctx->params) && packed != ctx->model_size)
			return ERRV(SRC_SIZE_MISMATCH);
	}
	if (model_needed(&ctx->params) && ctx->work_buf_size < packed)
		return ERRV(WORK_BUF_TOO_SMALL);
	if (!dst)
		return ERRV(DST_NULL);
	if ((uintptr_t)dst & 7u)
		return ERRV(DST_UNALIGNED);
	e = cmp_coder_resolve(p->enc, p->par, p->outlier_param, &p->outlier);
	if (is_err(e))
		return e;
	p->hdr_bytes = (p->pre == CMP_PREPROCESS_NONE && p->enc == CMP_ENCODER_UNCOMPRESSED) ? CMP_HDR_SIZE
											   : HDR_MAX_SIZE;
	/* header serialisation (header.c:24-67): original size, then the flush */
	if (packed > CMP_HDR_MAX_ORIGINAL_SIZE)
		return ERRV(HDR_ORIGINAL_TOO_LARGE);
	if (cap < p->hdr_bytes)
		return ERRV(DST_TOO_SMALL);
	/* preprocessing init (preprocess.c:321-393) */
	if (p->pre == CMP_PREPROCESS_IWT || p->pre == CMP_PREPROCESS_MODEL) {
		if (!ctx->work_buf)
			return ERRV(WORK_BUF_NULL);
		if (ctx->work_buf_size < ((packed + 1u) & ~1u))
			return ERRV(WORK_BUF_TOO_SMALL);
		if ((uintptr_t)ctx->work_buf & 1u)
			return ERRV(WORK_BUF_UNALIGNED);
	} else if (p->pre != CMP_PREPROCESS_NONE && p->pre != CMP_PREPROCESS_DIFF) {
		return ERRV(PARAMS_INVALID);
	}
	p->model_mode = model_needed(&ctx->params) ?
				(ctx->sequence_number == 0 ? AIRS_MODEL_STORE : AIRS_MODEL_UPDATE) :
				AIRS_MODEL_NONE;
	p->seq = ctx->sequence_number;
	return 0;
}

/* bit position whose flush fails for capacity cap: samples reaching it keep
 * their old model (cmp.c:300-302 breaks the loop before the model update) */
uint64_t model_fail_bit(uint32_t cap, uint32_t n)
{
	uint32_t bound = cmp_compress_bound(2u * n);

	if (!is_err(bound) && cap >= bound)
		return UINT64_MAX;
	return 64ull * (cap / 8u) + 63ull;
}

/* Longest codeword of a pass: 16 raw bits; GOLOMB_ZERO k + 17 with k =
 * floor(log2 g) (the escape, and the longest code below the outlier,
 * encoder.c:154-182; CMP_GPU_AUTO_RICE selects k up to 15); otherwise the
 * reference's own bound of 48 bits (encoder.c:381-386). */
static uint32_t pass_max_bits(uint32_t enc, uint32_t g, int auto_rice)
{
	uint32_t k = 0;

	if (enc == CMP_ENCODER_UNCOMPRESSED)
		return 16u;
	if (enc != CMP_ENCODER_GOLOMB_ZERO || !g)
		return 48u;
	if (auto_rice)
		return 32u;
	while ((2u << k) <= g)
		k++;
	return k + 17u;
}

/* can a frame of n samples of this context exceed the 24-bit size field? */
int size_field_can_overflow(const struct cmp_params *P, uint32_t n, uint32_t flags)
{
	uint32_t bits = pass_max_bits(P->primary_encoder_type, P->primary_encoder_param,
				      (flags & CMP_GPU_AUTO_RICE) != 0);

	if (P->secondary_iterations) {
		const uint32_t s = pass_max_bits(P->secondary_encoder_type, P->secondary_encoder_param, 0);

		bits = s > bits ? s : bits;
	}
	return HDR_MAX_SIZE + CMP_CHECKSUM_SIZE + ((uint64_t)n * bits + 7u) / 8u > CMP_HDR_MAX_COMPRESSED_SIZE;
}

/* largest possible frame for n samples: header + 48 bits/sample + checksum */
uint64_t frame_worst(uint32_t n)
{
	return HDR_MAX_SIZE + CMP_CHECKSUM_SIZE + payload_bound(2u * n) + 8u;
}

/* a launch's output capacity: the caller's, at most the largest possible frame */
uint32_t launch_cap(uint32_t cap, uint32_t n)
{
	return cap < frame_worst(n) ? cap : (uint32_t)frame_worst(n);
}

/* size of the raw (fallback) frame of a context, as cmp_compress_generic (cmp.c:342-393) */
uint32_t raw_frame_size(const struct cmp_context *ctx, uint32_t n)
{
	return CMP_HDR_SIZE + 2u * n + (ctx->params.checksum_enabled ? CMP_CHECKSUM_SIZE : 0u);
}

/* the uncompressed fallback's second attempt (cmp_compress_generic,
 * cmp.c:367-393): reset, then the prologue of the frame as NONE + UNCOMPRESSED
 * at the raw size */
uint32_t fallback_prologue(struct cmp_context *ctx, void *dst, uint32_t raw, uint32_t n, struct pass *p,
			   uint32_t *draws)
{
	const enum cmp_preprocessing save_pre = ctx->params.primary_preprocessing;
	const enum cmp_encoder_type save_enc = ctx->params.primary_encoder_type;
	uint32_t r = ctx_reset(ctx, draws);

	if (is_err(r))
		return r;
	ctx->params.primary_preprocessing = CMP_PREPROCESS_NONE;
	ctx->params.primary_encoder_type = CMP_ENCODER_UNCOMPRESSED;
	r = engine_prologue(ctx, dst, raw, n, p, draws);
	ctx->params.primary_preprocessing = save_pre;
	ctx->params.primary_encoder_type = save_enc;
	return r;
}

/* The launch as far as the batch, the pass, the context's parameters and the
 * capacity give it (everything else zero); the caller adds what is its own:
 * the frames, identifiers, model addressing, scratch pointers. */
void launch_fill(struct airs_launch *L, const struct cmp_gpu_batch *b, const struct batch_shape *sh,
		 const struct cmp_context *ctx, const struct pass *p, uint32_t cap)
{
	memset(L, 0, sizeof(*L));
	L->src = b->src;
	L->src_stride = b->src_stride;
	L->sample_bytes = sh->bytes;
	L->is_unsigned = sh->is_unsigned;
	L->n = sh->n;
	L->dst = b->dst;
	L->dst_stride = b->dst_stride;
	L->cap = launch_cap(cap, sh->n);
	L->preprocessing = p->pre;
	L->encoder_type = p->enc;
	L->encoder_param = p->par;
	L->outlier_param = p->outlier_param;
	L->model_mode = p->model_mode;
	L->model_rate = ctx->params.model_rate;
	/* a frame that runs out of room in a fallback-sized first attempt falls
	 * back, and the fallback stores the whole model: no fail bit needed */
	L->fail_bit = (ctx->params.uncompressed_fallback_enabled && cap == raw_frame_size(ctx, sh->n))
			      ? UINT64_MAX
			      : model_fail_bit(cap, sh->n);
	L->seq = p->seq;
	L->checksum_enabled = ctx->params.checksum_enabled ? 1u : 0u;
	L->status = b->sizes;
}

/* an internal failure of the host path (GENERIC), named on stderr */
static uint32_t host_fail(const char *what)
{
	fprintf(stderr, "airscmp: host path: %s failed (%s)\n", what, airs_dev_last_error());
	return ERRV(GENERIC);
}

/* Host-pointer frame: stage through device scratch, run, copy back.
 * fallback: the frame's second attempt (fallback_prologue). */
static uint32_t host_engine(struct cmp_context *ctx, void *dst, uint32_t cap, const struct frame_io *io, int fallback)
{
	const struct batch_shape sh = { io->bytes, io->n, 1, io->kind == KIND_U16 };
	struct pass p;
	struct airs_launch L;
	struct airs_dev_engine *dev;
	uint32_t e, st[2] = { 0, 0 };
	const uint32_t packed = 2u * io->n;
	void *d_src, *d_dst, *d_model = NULL, *d_status, *d_ck = NULL;

	e = fallback ? fallback_prologue(ctx, dst, cap, io->n, &p, NULL) : engine_prologue(ctx, dst, cap, io->n, &p, NULL);
	if (is_err(e))
		return e;
	dev = host_dev();
	if (!dev)
		return ERRV(GENERIC);

	d_src = airs_dev_scratch(dev, SLOT_SRC, (size_t)io->n * io->bytes);
	d_dst = airs_dev_scratch(dev, SLOT_DST, (size_t)frame_worst(io->n));
	d_status = airs_dev_scratch(dev, SLOT_STATUS, 64);
	if (!d_src || !d_dst || !d_status)
		return host_fail("device scratch");
	if (is_err(airs_dev_h2d(dev, d_src, io->src, (size_t)io->n * io->bytes)))
		return host_fail("sample upload");
	if (p.model_mode != AIRS_MODEL_NONE || p.pre == CMP_PREPROCESS_IWT) {
		/* the work buffer on the device: the model, or the IWT coefficients
		 * (computed there by the launch, so not uploaded) */
		d_model = airs_dev_scratch(dev, SLOT_MODEL, (size_t)packed + 16u);
		if (!d_model)
			return host_fail("model scratch");
		if (p.pre != CMP_PREPROCESS_IWT && is_err(airs_dev_h2d(dev, d_model, ctx->work_buf, packed)))
			return host_fail("model upload");
	}
	if (ctx->params.checksum_enabled) {
		d_ck = airs_dev_scratch(dev, SLOT_CK, 64);
		if (!d_ck || is_err(airs_dev_checksum(dev, d_src, 0, io->bytes, io->n, 1, NULL, d_ck)))
			return host_fail("checksum");
	}

	/* the staged frame, as a batch of one */
	const struct cmp_gpu_batch hb = { .src = d_src, .dst = d_dst, .sizes = d_status };

	launch_fill(&L, &hb, &sh, ctx, &p, cap);
	L.num_frames = 1;
	L.frame_mul = 1;
	L.model = d_model;
	L.model_div = 1;
	/* the fallback's second attempt is a launch of its own that reads the
	 * model back from work_buf: the first attempt keeps its fail bit */
	L.fail_bit = model_fail_bit(cap, io->n);
	L.id_base = ctx->identifier;
	L.checksums = d_ck;
	L.needed = (uint32_t *)d_status + 1;
	e = airs_dev_encode(dev, &L);
	if (cmp_get_error_code(e) == CMP_ERR_GENERIC)
		return host_fail("encode launch");
	if (is_err(e))
		return e;
	if (is_err(airs_dev_d2h(dev, st, d_status, sizeof(st))))
		return host_fail("status read-back");
	/* work_buf afterwards holds what the reference leaves there: the model,
	 * or the IWT coefficients (overwritten by the model where it is stored) */
	if (d_model && is_err(airs_dev_d2h(dev, ctx->work_buf, d_model, packed)))
		return host_fail("model read-back");
	if (is_err(airs_dev_sync(dev)))
		return host_fail("synchronisation");
	if (is_err(st[0]))
		return st[0];
	if (is_err(airs_dev_d2h(dev, dst, d_dst, st[0])) || is_err(airs_dev_sync(dev)))
		return host_fail("frame read-back");
	ctx->sequence_number++;
	return st[0];
}

/* uncompressed fallback (reference cmp_compress_generic, cmp.c:342-393) */
static uint32_t host_generic(struct cmp_context *ctx, void *dst, uint32_t cap, const struct frame_io *io)
{
	uint32_t raw, r;

	if (!ctx)
		return ERRV(GENERIC);
	if (ctx->magic != CTX_MAGIC)
		return ERRV(CONTEXT_INVALID);
	if (is_err(cap))
		return ERRV(GENERIC);
	raw = raw_frame_size(ctx, io->n);
	if (!ctx->params.uncompressed_fallback_enabled || cap < raw)
		return host_engine(ctx, dst, cap, io, 0);
	r = host_engine(ctx, dst, raw, io, 0);
	return cmp_get_error_code(r) == CMP_ERR_DST_TOO_SMALL ? host_engine(ctx, dst, raw, io, 1) : r;
}

static uint32_t host_compress(struct cmp_context *ctx, void *dst, uint32_t cap, const void *src,
			      uint32_t size, enum sample_kind kind)
{
	struct frame_io io;
	uint32_t stride = kind == KIND_I16_IN_I32 ? 4u : 2u, r;

	/* reference sample_reader.h:19-51 */
	if (!src)
		return ERRV(SRC_NULL);
	if (size == 0 || size % stride)
		return ERRV(SRC_SIZE_WRONG);
	memset(&io, 0, sizeof(io));
	io.src = src;
	io.n = size / stride;
	io.bytes = stride;
	io.kind = kind;
	pthread_mutex_lock(&g_host_lock);
	r = host_generic(ctx, dst, cap, &io);
	pthread_mutex_unlock(&g_host_lock);
	return r;
}

uint32_t cmp_compress_u16(struct cmp_context *ctx, void *dst, uint32_t dst_capacity, const uint16_t *src,
			  uint32_t src_size)
{
	return host_compress(ctx, dst, dst_capacity, src, src_size, KIND_U16);
}

uint32_t cmp_compress_i16(struct cmp_context *ctx, void *dst, uint32_t dst_capacity, const int16_t *src,
			  uint32_t src_size)
{
	return host_compress(ctx, dst, dst_capacity, src, src_size, KIND_I16);
}

uint32_t cmp_compress_i16_in_i32(struct cmp_context *ctx, void *dst, uint32_t dst_capacity,
				 const int32_t *src, uint32_t src_size)
{
	return host_compress(ctx, dst, dst_capacity, src, src_size, KIND_I16_IN_I32);
}

/* ================================================================== */
/* device batch API (cmp_gpu.h)                                       */
/* ================================================================== */

uint32_t cmp_gpu_decompress(struct cmp_gpu_engine *engine, const struct cmp_gpu_decode_batch *b)
{
	if (!engine || !b || !b->src || !b->dst || !b->status || !b->num_frames || b->num_frames > 65535u)
		return ERRV(GENERIC);
	if (((uintptr_t)b->src & 7u) || (b->src_stride & 7u) || b->src_capacity < HDR_MAX_SIZE ||
	    (b->src_capacity & 3u) || (b->num_frames > 1 && b->src_stride < b->src_capacity))
		return ERRV(GENERIC);
	if (b->model && (((uintptr_t)b->model & 1u) || (b->model_stride & 1u)))
		return ERRV(GENERIC);
	return airs_dev_decode(engine->dev, b->src, b->src_stride, b->src_capacity, b->num_frames, b->dst,
			       b->dst_stride, b->dst_samples, b->status, b->model, b->model_stride);
}

int cmp_gpu_available(void)
{
	return airs_dev_available();
}

uint32_t cmp_gpu_engine_create(struct cmp_gpu_engine **engine, void *hip_stream)
{
	struct cmp_gpu_engine *g;

	if (!engine)
		return ERRV(GENERIC);
	*engine = NULL;
	g = calloc(1, sizeof(*g));
	if (!g)
		return ERRV(GENERIC);
	g->dev = airs_dev_engine_create(hip_stream);
	if (!g->dev) {
		fprintf(stderr, "airscmp: cannot create GPU engine (%s)\n", airs_dev_last_error());
		free(g);
		return ERRV(GENERIC);
	}
	*engine = g;
	return 0;
}

uint32_t cmp_gpu_engine_set_option(struct cmp_gpu_engine *engine, uint32_t option, uint32_t value)
{
	if (!engine)
		return ERRV(GENERIC);
	if (option == CMP_GPU_OPT_IMAGE_CHUNK) { /* a host-side plan: the device layer never sees it */
		engine->image_chunk = value;
		return 0;
	}
	if (option == CMP_GPU_OPT_IMAGE_RAGGED) { /* how cmp_gpu_compress_image schedules: host-side too */
		engine->image_ragged = value;
		return 0;
	}
	if (option == CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM) { /* whether that schedule takes checksum-enabled contexts */
		if (value > 1u)
			return ERRV(PARAMS_INVALID);
		engine->image_ragged_ck = value;
		return 0;
	}
	return airs_dev_set_option(engine->dev, option, value);
}

void cmp_gpu_engine_destroy(struct cmp_gpu_engine *engine)
{
	if (!engine)
		return;
	airs_dev_engine_destroy(engine->dev);
	free(engine);
}

uint32_t cmp_gpu_synchronize(struct cmp_gpu_engine *engine)
{
	if (!engine)
		return ERRV(GENERIC);
	return airs_dev_sync(engine->dev);
}

uint32_t cmp_gpu_encode_stream(struct cmp_gpu_engine *engine, enum cmp_gpu_sample_type type, const void *src,
			       uint32_t num_samples, enum cmp_preprocessing preprocessing,
			       enum cmp_encoder_type encoder_type, uint32_t encoder_param, uint32_t encoder_outlier,
			       void *dst, uint32_t dst_capacity, uint32_t *size)
{
	const uint32_t bytes = type == CMP_GPU_I16_IN_I32 ? 4u : 2u;
	uint32_t e, outlier = 0;

	if (!engine || !size)
		return ERRV(GENERIC);
	if ((unsigned)type > CMP_GPU_I16_IN_I32)
		return ERRV(PARAMS_INVALID);
	if (!src)
		return ERRV(SRC_NULL);
	if (num_samples == 0 || num_samples > AIRS_STREAM_MAX)
		return ERRV(SRC_SIZE_WRONG);
	if ((uintptr_t)src % bytes) {
		fprintf(stderr, "airscmp: cmp_gpu_encode_stream: src must be %u-byte aligned\n", bytes);
		return ERRV(GENERIC);
	}
	if (!dst)
		return ERRV(DST_NULL);
	if ((uintptr_t)dst & 7u)
		return ERRV(DST_UNALIGNED);
	if (is_err(dst_capacity))
		return ERRV(GENERIC);
	if (preprocessing != CMP_PREPROCESS_NONE && preprocessing != CMP_PREPROCESS_DIFF)
		return ERRV(PARAMS_INVALID);
	/* the encoder's own checks (encoder.c:185-224) */
	e = cmp_coder_resolve(encoder_type, encoder_param, encoder_outlier, &outlier);
	if (is_err(e))
		return e;
	return airs_dev_encode_stream(engine->dev, src, bytes, num_samples, preprocessing, encoder_type,
				      encoder_type == CMP_ENCODER_UNCOMPRESSED ? 1u : encoder_param, encoder_outlier,
				      dst, dst_capacity, size);
}

uint32_t cmp_gpu_pack_frames(struct cmp_gpu_engine *engine, const void *frames, uint64_t frame_stride,
			     uint32_t frame_capacity, const uint32_t *sizes, uint32_t num_frames, void *out,
			     uint64_t *offsets)
{
	if (!engine || !frames || !sizes || !out || !offsets || !num_frames)
		return ERRV(GENERIC);
	if ((frame_stride & 7u) || ((uintptr_t)frames & 7u) || ((uintptr_t)out & 7u) ||
	    (num_frames > 1 && frame_stride < frame_capacity))
		return ERRV(DST_UNALIGNED);
	return airs_dev_pack_frames(engine->dev, frames, frame_stride, frame_capacity, sizes, num_frames,
				    ERRV(MAX_CODE), out, offsets);
}

uint32_t cmp_gpu_synthesize(struct cmp_gpu_engine *engine, void *dst, uint32_t sample_bytes, uint64_t seed,
			    uint32_t frame0, uint32_t samples_per_frame, uint32_t num_frames, uint64_t stride,
			    uint32_t noise_w)
{
	if (!engine || !dst || (sample_bytes != 2 && sample_bytes != 4))
		return ERRV(GENERIC);
	return airs_dev_synth(engine->dev, dst, sample_bytes, seed, frame0, samples_per_frame, num_frames,
			      stride, noise_w);
}
