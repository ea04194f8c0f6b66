/*
 * dev_stub.c -- TEST ONLY.  A host-memory stand-in for the HIP device layer
 * (airs_dev.h), so that the C host library (cmp_host.c, cmp_batch.c: parameter checks,
 * the context state machine, the batch planner and its step-by-step
 * fallback path) and the CLI parser can run under AddressSanitizer and
 * UndefinedBehaviorSanitizer on a machine without a GPU (SURVEY.md section 5,
 * sanitizer row).  It does not encode anything: an "encode" writes a
 * deterministic pseudo-random outcome per frame (a size that fits, or
 * CMP_ERR_DST_TOO_SMALL) plus a header-shaped first 16 bytes, which is
 * enough to drive every branch of the planner.  The walk (airs_dev_walk)
 * refuses and fails as the device does where the planner depends on it: the
 * fallback on the chip only for the context walk's batches, and without it
 * DST_TOO_SMALL for a frame past the capacity, so all three MODEL batch paths
 * and the redo of a context run.  Device memory is malloc'd host memory,
 * copies are memcpy.  Never linked into the product.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "airs_dev.h"

#define ERRV(code) ((uint32_t)0u - (uint32_t)(code))

struct airs_dev_engine {
	void *scratch[AIRS_NSLOT];
	size_t cap[AIRS_NSLOT];
	void *pinned;
	size_t pinned_cap;
	uint64_t salt;
	uint64_t coll[AIRS_COLL_WORDS]; /* the last two: the poison record */
};

/* failure injection for the multi-rank gather harness (gather_sim.c): the
 * scratch slot whose allocation fails on this thread (-1: none) */
__thread int stub_scratch_fail_slot = -1;
/* ... and the airs_dev_h2d on this thread that fails and copies nothing:
 * the k-th from now (1: the next one; 0: none) */
__thread int stub_h2d_fail_at;

uint64_t *airs_dev_coll(struct airs_dev_engine *e)
{
	return e ? e->coll : NULL;
}

/* Two 64-bit FNV-1a digests of what the host code asks of the device layer on
 * this thread, folded field by field in call order (never over a struct's
 * bytes, and never an address: a pointer enters as "is it NULL").  The launch
 * digest covers what every launch-like call is handed and what the device
 * would resolve per frame from it; the traffic digest covers scratch
 * requests, copies and synchronisations.  host_fuzz.c prints both. */
#define FNV_INIT 0xCBF29CE484222325ull
__thread uint64_t stub_launch_digest = FNV_INIT;
__thread uint64_t stub_traffic_digest = FNV_INIT;

static void fnv(uint64_t *d, uint64_t v)
{
	for (int i = 0; i < 8; i++, v >>= 8)
		*d = (*d ^ (v & 0xFFu)) * 0x100000001B3ull;
}

#define LD(v) fnv(&stub_launch_digest, (uint64_t)(v))
#define LDP(p) fnv(&stub_launch_digest, (p) != NULL)
#define TD(v) fnv(&stub_traffic_digest, (uint64_t)(v))
enum { TAG_ENCODE = 1, TAG_WALK, TAG_WALK_SUPPORTED, TAG_FB_STEP, TAG_FB_COPY, TAG_CHECKSUM, TAG_SELECT_RICE,
       TAG_PATCH_IDS, TAG_COMMIT_BEGIN, TAG_COMMIT_WAIT, TAG_COMMIT_RELEASE,
       TAG_SCRATCH, TAG_HOST_SCRATCH, TAG_H2D, TAG_D2H, TAG_MEMSET, TAG_D2D_ROWS, TAG_SYNC };

static uint64_t mix(uint64_t z)
{
	z += 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

int airs_dev_available(void)
{
	return 1;
}

const char *airs_dev_last_error(void)
{
	return "stub";
}

struct airs_dev_engine *airs_dev_engine_create(void *stream)
{
	struct airs_dev_engine *e = calloc(1, sizeof(struct airs_dev_engine));

	(void)stream;
	if (e)
		e->coll[AIRS_COLL_POISON] = ERRV(1u); /* CMP_ERR_GENERIC, as the device layer's create */
	return e;
}

uint32_t airs_dev_set_option(struct airs_dev_engine *e, uint32_t option, uint32_t value)
{
	if (!e)
		return (uint32_t)0 - 1u;
	if (option < AIRS_OPT_EXCLUSIVE || option > AIRS_OPT_NO_CONTEXT_WALK)
		return (uint32_t)0 - 10u;
	(void)value;
	return 0;
}

void airs_dev_engine_destroy(struct airs_dev_engine *e)
{
	if (!e)
		return;
	for (int i = 0; i < AIRS_NSLOT; i++)
		free(e->scratch[i]);
	free(e->pinned);
	free(e);
}

void *airs_dev_engine_stream(struct airs_dev_engine *e)
{
	(void)e;
	return NULL;
}

void *airs_dev_scratch(struct airs_dev_engine *e, int slot, size_t bytes)
{
	TD(TAG_SCRATCH), TD(slot), TD(bytes);
	if (!e || slot < 0 || slot >= AIRS_NSLOT || slot == stub_scratch_fail_slot)
		return NULL;
	if (bytes > e->cap[slot]) {
		free(e->scratch[slot]);
		e->scratch[slot] = malloc(bytes);
		e->cap[slot] = e->scratch[slot] ? bytes : 0;
	}
	return e->scratch[slot];
}

void *airs_dev_host_scratch(struct airs_dev_engine *e, size_t bytes)
{
	TD(TAG_HOST_SCRATCH), TD(bytes);
	if (!e)
		return NULL;
	if (bytes > e->pinned_cap) {
		free(e->pinned);
		e->pinned = malloc(bytes);
		e->pinned_cap = e->pinned ? bytes : 0;
	}
	return e->pinned;
}

/* the model of launch frame j (batch frame f), whichever form was passed */
static uint8_t *launch_model(const struct airs_launch *L, uint32_t j, uint32_t f)
{
	if (L->model_ptrs)
		return (uint8_t *)(uintptr_t)L->model_ptrs[j];
	return (uint8_t *)L->model + (uint64_t)(f / (L->model_div ? L->model_div : 1u)) * L->model_stride;
}

/* A model's place without its address: inside the engine's scratch (the
 * coefficients of batch_iwt) the slot and the offset in it, otherwise the byte
 * distance from the first such model of the launch (*base). */
static void fold_model(const struct airs_dev_engine *e, const uint8_t *m, const uint8_t **base)
{
	for (int i = 0; i < AIRS_NSLOT; i++)
		if (e->scratch[i] && m >= (const uint8_t *)e->scratch[i] && m < (const uint8_t *)e->scratch[i] + e->cap[i]) {
			LD(1), LD(i), LD(m - (const uint8_t *)e->scratch[i]);
			return;
		}
	if (!*base)
		*base = m;
	LD(0), LD(m - *base);
}

static void fold_launch(const struct airs_launch *L)
{
	LD(TAG_ENCODE);
	LDP(L->src), LD(L->src_stride), LD(L->sample_bytes), LD(L->is_unsigned), LD(L->n), LD(L->num_frames);
	LDP(L->frame_list), LD(L->frame_add), LD(L->frame_mul);
	LDP(L->dst), LD(L->dst_stride), LD(L->cap);
	LD(L->preprocessing), LD(L->encoder_type), LD(L->encoder_param), LD(L->outlier_param);
	LDP(L->frame_g), LD(L->auto_rice), LDP(L->frame_g_scratch);
	LDP(L->model), LD(L->model_stride), LD(L->model_div), LDP(L->model_ptrs), LD(L->model_ptrs_al16);
	LD(L->model_mode), LD(L->model_rate), LD(L->fail_bit);
	LDP(L->seqs), LD(L->id_base), LD(L->id_step), LDP(L->ids), LD(L->seq);
	LD(L->checksum_enabled), LDP(L->checksums), LDP(L->status), LDP(L->needed);
}

uint32_t airs_dev_encode(struct airs_dev_engine *e, const struct airs_launch *L)
{
	const uint8_t *model0 = NULL;

	if (L)
		fold_launch(L);
	if (!e || !L || !L->n || !L->num_frames || !L->status)
		return ERRV(1u);
	for (uint32_t j = 0; j < L->num_frames; j++) {
		const uint32_t f = L->frame_list ? L->frame_list[j] : L->frame_add + j * L->frame_mul;
		if (f == 0xFFFFFFFFu) /* AIRS_NO_FRAME: a hole in a device-planned list */
			continue;
		/* what the device resolves for this frame */
		LD(f), LD(L->ids ? L->ids[j] : L->id_base + j * L->id_step);
		if (L->seqs)
			LD(L->seqs[f]);
		if (L->model || L->model_ptrs)
			fold_model(e, launch_model(L, j, f), &model0);
		if (L->checksum_enabled && L->checksums)
			LD(L->checksums[f]);
		const uint64_t h = mix(e->salt++ ^ ((uint64_t)f << 32) ^ L->n);
		/* every input byte the kernel would read is read here too */
		const uint8_t *src = (const uint8_t *)L->src + (uint64_t)f * L->src_stride;
		volatile uint8_t sink = src[0] ^ src[(uint64_t)L->n * L->sample_bytes - 1u];
		(void)sink;
		uint32_t size = 16u + (uint32_t)(h % (3ull * L->n + 8u));
		uint8_t *dst = (uint8_t *)L->dst + (uint64_t)f * L->dst_stride;
		if (L->model_mode != AIRS_MODEL_NONE) {
			uint8_t *m = launch_model(L, j, f);
			m[0] ^= 1u; /* touch both ends of the model */
			m[2u * L->n - 1u] ^= 1u;
		}
		if (L->checksum_enabled && L->checksums)
			(void)L->checksums[f];
		if (L->frame_g)
			(void)L->frame_g[f];
		if (size > L->cap) {
			L->status[f] = ERRV(30u); /* DST_TOO_SMALL */
		} else {
			memset(dst, 0, 16);
			dst[0] = (uint8_t)(size >> 16);
			dst[1] = (uint8_t)(size >> 8);
			dst[2] = (uint8_t)size;
			dst[size - 1u] = 0x5A;
			L->status[f] = size;
		}
		if (L->needed)
			L->needed[f] = size;
	}
	return 0;
}

/* The device resolves the fallback on the chip (w->fb) only in the context
 * walk: frames of that walk's size and enough contexts to fill the CUs
 * (ctx_walk_words, encode.hip).  These two stand in for that rule at the
 * harness's sizes, so that the host's fall-through from batch_walk_fb to
 * batch_walk_spec is exercised as written. */
#define STUB_CTX_WALK_SAMPLES 8192u
#define STUB_CTX_WALK_MIN_CTX 3u

/* the walk needs n % 4096 == 0 and 16-byte aligned inputs; the stub checks
 * the same so that the host's applicability test is exercised as written */
static void fold_walk(uint32_t tag, const struct airs_walk *w)
{
	LD(tag);
	LDP(w->src), LD(w->src_stride), LD(w->sample_bytes), LD(w->is_unsigned), LD(w->n), LD(w->num_ctx), LD(w->fpc);
	LDP(w->dst), LD(w->dst_stride), LD(w->cap);
	LDP(w->model), LD(w->model_stride), LDP(w->model_ptrs);
	LD(w->pre_p), LD(w->enc_p), LD(w->g_p), LD(w->outl_p), LD(w->enc_s), LD(w->g_s), LD(w->outl_s);
	LD(w->model_rate), LD(w->iters), LD(w->seq0), LDP(w->seq0s);
	LD(w->id_base), LD(w->id_cstep), LD(w->id_astep), LDP(w->ids);
	LD(w->checksum_enabled), LDP(w->checksums), LDP(w->status);
	LD(w->fb), LD(w->raw_size), LDP(w->draws), LDP(w->seq_out);
}

static int walk_ok(const struct airs_walk *w)
{
	if (!w || !w->n || w->n % 4096u || !w->num_ctx || !w->fpc || (w->sample_bytes != 2 && w->sample_bytes != 4))
		return 0;
	if (((uintptr_t)w->src & 15u) || (w->src_stride & 15u))
		return 0;
	if (w->fb && (!w->draws || !w->seq_out || w->cap != w->raw_size || w->n != STUB_CTX_WALK_SAMPLES ||
		      w->num_ctx < STUB_CTX_WALK_MIN_CTX))
		return 0;
	return w->model_ptrs || !(((uintptr_t)w->model & 15u) || (w->model_stride & 15u));
}

int airs_dev_walk_supported(const struct airs_walk *w)
{
	const int ok = walk_ok(w);

	if (w)
		fold_walk(TAG_WALK_SUPPORTED, w);
	LD(ok);
	return ok;
}

unsigned long stub_walk_calls;

uint32_t airs_dev_walk(struct airs_dev_engine *e, struct airs_walk *w)
{
	const uint8_t *model0 = NULL;

	if (w)
		fold_walk(TAG_WALK, w);
	if (!e || !walk_ok(w) || !w->status)
		return ERRV(10u);
	stub_walk_calls++;
	for (uint32_t c = 0; c < w->num_ctx; c++) {
		uint8_t *m = w->model_ptrs ? (uint8_t *)(uintptr_t)w->model_ptrs[c]
					   : (uint8_t *)w->model + (uint64_t)c * w->model_stride;
		m[0] ^= 1u; /* touch both ends of the model */
		m[2u * w->n - 1u] ^= 1u;
		if (w->seq0s)
			(void)w->seq0s[c];
		for (uint32_t a = 0; a < w->fpc; a++) {
			const uint32_t f = c * w->fpc + a;
			const uint64_t h = mix(e->salt++ ^ ((uint64_t)f << 32) ^ w->n);
			const uint8_t *src = (const uint8_t *)w->src + (uint64_t)f * w->src_stride;
			volatile uint8_t sink = src[0] ^ src[(uint64_t)w->n * w->sample_bytes - 1u];
			(void)sink;
			uint32_t size = 16u + (uint32_t)(h % (3ull * w->n + 8u));
			uint8_t *dst = (uint8_t *)w->dst + (uint64_t)f * w->dst_stride;
			/* what the device resolves for this frame */
			LD(f), LD(w->ids ? w->ids[f] : w->id_base + c * w->id_cstep + a * w->id_astep);
			if (w->seq0s)
				LD(w->seq0s[c]);
			fold_model(e, m, &model0);
			if (w->checksum_enabled && w->checksums)
				LD(w->checksums[f]);
			if (size > w->cap) {
				/* the segment walk reports a frame that did not fit (the
				 * host runs its context again); with fb the walk resolves
				 * the fallback itself and every frame has a size.  In the
				 * asynchronous mode cap is at least the frame bound,
				 * 26 + 6n, above the largest size here, 16 + 3n + 7. */
				if (!w->fb) {
					w->status[f] = ERRV(30u); /* DST_TOO_SMALL */
					continue;
				}
				size = w->cap;
			}
			memset(dst, 0, 16);
			dst[size - 1u] = 0x5A;
			w->status[f] = size;
			if (w->fb) /* the walk's fallback: identifier draws of the frame */
				w->draws[f] = (uint8_t)(h >> 40) & 3u;
		}
		if (w->fb)
			w->seq_out[c] = (uint8_t)(1u + c % 3u);
	}
	return 0;
}

uint32_t airs_dev_encode_stream(struct airs_dev_engine *e, const void *src, uint32_t sample_bytes, uint32_t n,
				uint32_t preprocessing, uint32_t encoder_type, uint32_t encoder_param,
				uint32_t outlier_param, void *dst, uint32_t cap, uint32_t *status)
{
	(void)preprocessing, (void)encoder_type, (void)encoder_param, (void)outlier_param;
	if (!e || !n)
		return ERRV(1u);
	volatile uint8_t sink = ((const uint8_t *)src)[(uint64_t)n * sample_bytes - 1u];
	(void)sink;
	const uint32_t size = 1u + (uint32_t)(mix(e->salt++) % (3ull * n));
	if (size > cap) {
		*status = ERRV(30u);
	} else {
		((uint8_t *)dst)[size - 1u] = 0x5A;
		*status = size;
	}
	return 0;
}

uint32_t airs_dev_pack_frames(struct airs_dev_engine *e, const void *src, uint64_t src_stride,
			      uint32_t max_frame_bytes, const uint32_t *sizes, uint32_t num_frames,
			      uint32_t err_floor, void *out, uint64_t *offsets)
{
	uint64_t o = 0;
	(void)e, (void)max_frame_bytes;
	for (uint32_t f = 0; f < num_frames; f++) {
		const uint32_t sz = sizes[f] > err_floor ? 0u : sizes[f];
		offsets[f] = o;
		memcpy((uint8_t *)out + o, (const uint8_t *)src + (uint64_t)f * src_stride, sz);
		o += ((uint64_t)sz + 7u) & ~7ull;
	}
	offsets[num_frames] = o;
	return 0;
}

/* the per-context state machine of fb_step_kernel (encode.hip), on the host */
static void fold_fb(uint32_t tag, const struct airs_fb_step *a)
{
	LD(tag);
	LDP(a->state), LD(a->num_ctx), LD(a->fpc), LD(a->prev), LD(a->cur), LD(a->packed), LD(a->iters);
	LD(a->model_needed), LD(a->fb_eligible), LD(a->raw_size);
	LD(a->err_floor), LD(a->err_small), LD(a->err_mismatch), LD(a->err_too_large);
	LDP(a->flist_p), LDP(a->flist_s), LDP(a->seqs), LDP(a->draws), LDP(a->kind), LDP(a->fb), LDP(a->status);
	LDP(a->src), LD(a->src_stride), LD(a->sample_bytes), LD(a->n), LDP(a->dst), LD(a->dst_stride);
	LDP(a->checksums), LD(a->checksum), LDP(a->model), LD(a->model_stride), LDP(a->model_ptrs);
}

static uint8_t *fb_model(const struct airs_fb_step *a, uint32_t c)
{
	return a->model_ptrs ? (uint8_t *)(uintptr_t)a->model_ptrs[c] : (uint8_t *)a->model + (uint64_t)c * a->model_stride;
}

uint32_t airs_dev_fb_step(struct airs_dev_engine *e, const struct airs_fb_step *a)
{
	if (a)
		fold_fb(TAG_FB_STEP, a);
	if (!e || !a || !a->num_ctx)
		return ERRV(1u);
	for (uint32_t c = 0; c < a->num_ctx; c++) /* the states the step starts from */
		LD(a->state[2u * c]), LD(a->state[2u * c + 1u]);
	for (uint32_t c = 0; c < a->num_ctx; c++) {
		uint32_t seq = a->state[2u * c], msize = a->state[2u * c + 1u];
		if (a->prev >= 0) {
			const uint32_t f = c * a->fpc + (uint32_t)a->prev;
			uint8_t fb = 0;
			if (a->kind[f]) {
				const uint32_t v = a->status[f];
				if (v <= a->err_floor) {
					seq++;
				} else if (a->fb_eligible && v == a->err_small) {
					fb = 1;
					a->draws[f] = (uint8_t)(a->draws[f] + 2u);
					msize = a->packed;
					a->status[f] = a->raw_size > 0xFFFFFFu ? a->err_too_large : a->raw_size;
					seq = a->raw_size > 0xFFFFFFu ? 0u : 1u;
				}
			}
			a->fb[f] = fb;
		}
		if (a->cur >= 0) {
			const uint32_t f = c * a->fpc + (uint32_t)a->cur;
			uint32_t lp = 0xFFFFFFFFu, ls = 0xFFFFFFFFu;
			uint8_t kind = 0, draws = 0;
			if (seq == 0 || seq > a->iters) {
				seq = 0;
				msize = a->packed;
				draws = 1;
				kind = 1;
				lp = f;
			} else if (a->model_needed && msize != a->packed) {
				a->status[f] = a->err_mismatch;
			} else {
				kind = 2;
				ls = f;
			}
			a->flist_p[c] = lp;
			a->flist_s[c] = ls;
			a->seqs[f] = (uint8_t)seq;
			a->kind[f] = kind;
			a->draws[f] = draws;
		}
		a->state[2u * c] = seq;
		a->state[2u * c + 1u] = msize;
	}
	return 0;
}

/* fb_copy_kernel: raw frames of the previous step's fallbacks */
uint32_t airs_dev_fb_copy(struct airs_dev_engine *e, const struct airs_fb_step *a)
{
	const uint8_t *model0 = NULL;

	if (a)
		fold_fb(TAG_FB_COPY, a);
	if (!e || !a || !a->num_ctx || a->prev < 0 || !a->n)
		return ERRV(1u);
	for (uint32_t c = 0; c < a->num_ctx; c++) {
		const uint32_t f = c * a->fpc + (uint32_t)a->prev;
		if (!a->fb[f])
			continue;
		const uint8_t *fs = (const uint8_t *)a->src + (uint64_t)f * a->src_stride;
		uint8_t *fd = (uint8_t *)a->dst + (uint64_t)f * a->dst_stride;
		uint16_t *fm = NULL;
		LD(f);
		if (a->model_needed) {
			fm = (uint16_t *)fb_model(a, c);
			fold_model(e, (const uint8_t *)fm, &model0);
		}
		if (a->checksum)
			LD(a->checksums[f]);
		memset(fd, 0, 16);
		for (uint32_t i = 0; i < a->n; i++) {
			const uint16_t x = a->sample_bytes == 2 ? ((const uint16_t *)fs)[i]
							       : (uint16_t)((const uint32_t *)fs)[i];
			fd[16u + 2u * i] = (uint8_t)(x >> 8);
			fd[17u + 2u * i] = (uint8_t)x;
			if (fm)
				fm[i] = x;
		}
		if (a->checksum)
			memcpy(fd + 16u + 2u * a->n, &a->checksums[f], 4);
	}
	return 0;
}

uint32_t airs_dev_checksum(struct airs_dev_engine *e, const void *src, uint64_t src_stride, uint32_t sample_bytes,
			   uint32_t n, uint32_t num_frames, const uint32_t *frame_list, uint32_t *out)
{
	LD(TAG_CHECKSUM), LDP(src), LD(src_stride), LD(sample_bytes), LD(n), LD(num_frames), LDP(frame_list), LDP(out);
	if (!e || !n || !num_frames)
		return ERRV(1u);
	for (uint32_t j = 0; j < num_frames; j++) {
		const uint32_t f = frame_list ? frame_list[j] : j;
		const uint8_t *s = (const uint8_t *)src + (uint64_t)f * src_stride;
		LD(f);
		out[frame_list ? f : j] = s[0] + s[(uint64_t)n * sample_bytes - 1u];
	}
	return 0;
}

uint32_t airs_dev_select_rice(struct airs_dev_engine *e, const void *src, uint64_t src_stride,
			      uint32_t sample_bytes, uint32_t n, uint32_t num_frames, const uint32_t *frame_list,
			      uint32_t frame_add, uint32_t frame_mul, uint32_t preprocessing, uint32_t *out_g)
{
	(void)e;
	LD(TAG_SELECT_RICE), LDP(src), LD(src_stride), LD(sample_bytes), LD(n), LD(num_frames), LDP(frame_list);
	LD(frame_add), LD(frame_mul), LD(preprocessing), LDP(out_g);
	for (uint32_t j = 0; j < num_frames; j++) {
		const uint32_t f = frame_list ? frame_list[j] : frame_add + j * frame_mul;
		if (f != 0xFFFFFFFFu) {
			LD(f);
			out_g[f] = 32u;
		}
	}
	return 0;
}

uint32_t airs_dev_synth(struct airs_dev_engine *e, void *dst, uint32_t sample_bytes, uint64_t seed, uint32_t frame0,
			uint32_t n, uint32_t num_frames, uint64_t stride, uint32_t W)
{
	(void)e, (void)W;
	for (uint32_t f = 0; f < num_frames; f++)
		for (uint32_t i = 0; i < n * sample_bytes; i++)
			((uint8_t *)dst)[(uint64_t)f * stride + i] = (uint8_t)mix(seed + frame0 + f + i);
	return 0;
}

uint32_t airs_dev_patch_ids(struct airs_dev_engine *e, void *dst, uint64_t dst_stride, uint32_t num_frames,
			    uint32_t frame_add, uint32_t frame_mul, const uint64_t *ids, const uint32_t *status)
{
	(void)e;
	LD(TAG_PATCH_IDS), LDP(dst), LD(dst_stride), LD(num_frames), LD(frame_add), LD(frame_mul), LDP(ids), LDP(status);
	for (uint32_t j = 0; j < num_frames; j++) {
		const uint32_t f = frame_add + j * frame_mul;
		LD(ids[j]);
		if (status && status[f] > ERRV(128u))
			continue;
		for (int b = 0; b < 6; b++)
			((uint8_t *)dst)[(uint64_t)f * dst_stride + 8u + (uint32_t)b] = (uint8_t)(ids[j] >> (40 - 8 * b));
	}
	return 0;
}

uint32_t airs_dev_decode(struct airs_dev_engine *e, const void *src, uint64_t src_stride, uint32_t src_cap,
			 uint32_t num_frames, uint16_t *dst, uint64_t dst_stride, uint32_t dst_samples,
			 uint32_t *status, const uint16_t *model, uint64_t model_stride)
{
	(void)e, (void)dst, (void)dst_stride, (void)dst_samples, (void)model, (void)model_stride;
	for (uint32_t f = 0; f < num_frames; f++) {
		const uint8_t *s = (const uint8_t *)src + (uint64_t)f * src_stride;
		status[f] = src_cap ? s[0] + 0u * s[src_cap - 1u] : 0u;
	}
	return 0;
}

void *airs_dev_malloc(size_t bytes)
{
	return malloc(bytes ? bytes : 1);
}

void airs_dev_free(void *p)
{
	free(p);
}

uint32_t airs_dev_h2d(struct airs_dev_engine *e, void *dst, const void *src, size_t bytes)
{
	(void)e;
	TD(TAG_H2D), TD(bytes);
	if (stub_h2d_fail_at && --stub_h2d_fail_at == 0)
		return ERRV(1u);
	memcpy(dst, src, bytes);
	return 0;
}

uint32_t airs_dev_d2h(struct airs_dev_engine *e, void *dst, const void *src, size_t bytes)
{
	(void)e;
	TD(TAG_D2H), TD(bytes);
	memcpy(dst, src, bytes);
	return 0;
}

uint32_t airs_dev_sync(struct airs_dev_engine *e)
{
	(void)e;
	TD(TAG_SYNC);
	return 0;
}

static uint8_t g_commit_flags[8192];

uint32_t airs_dev_memset(struct airs_dev_engine *e, void *dst, int v, size_t bytes)
{
	(void)e;
	TD(TAG_MEMSET), TD(v), TD(bytes);
	memset(dst, v, bytes);
	return 0;
}

uint32_t airs_dev_d2d_rows(struct airs_dev_engine *e, void *dst, size_t dpitch, const void *src, size_t spitch,
			   size_t width, size_t rows)
{
	(void)e;
	TD(TAG_D2D_ROWS), TD(dpitch), TD(spitch), TD(width), TD(rows);
	for (size_t r = 0; r < rows; r++)
		memmove((uint8_t *)dst + r * dpitch, (const uint8_t *)src + r * spitch, width);
	return 0;
}

uint32_t airs_dev_commit_begin(struct airs_dev_engine *e, const uint32_t *status, uint32_t num_ctx, uint32_t fpc,
			       void *dst, uint64_t dst_stride, uint32_t *seq)
{
	(void)e;
	LD(TAG_COMMIT_BEGIN), LDP(status), LD(num_ctx), LD(fpc), LDP(dst), LD(dst_stride), LDP(seq);
	for (uint32_t c = 0; c < num_ctx && c < sizeof(g_commit_flags); c++) {
		uint32_t any = 0;
		for (uint32_t a = 0; a < fpc; a++)
			any |= status[(size_t)c * fpc + a] > 0xFFFFFFFFu - 128u;
		g_commit_flags[c] = (uint8_t)any;
	}
	*seq = 1;
	return 0;
}

uint32_t airs_dev_commit_wait(struct airs_dev_engine *e, uint32_t seq, uint32_t num_ctx, uint8_t *flags)
{
	(void)e;
	LD(TAG_COMMIT_WAIT), LD(seq), LD(num_ctx), LDP(flags);
	memcpy(flags, g_commit_flags, num_ctx < sizeof(g_commit_flags) ? num_ctx : sizeof(g_commit_flags));
	return 0;
}

int airs_dev_commit_release(struct airs_dev_engine *e, uint32_t seq, const uint64_t *ids, uint32_t total)
{
	(void)e;
	LD(TAG_COMMIT_RELEASE), LD(seq), LD(total), LDP(ids);
	for (uint32_t f = 0; ids && f < total; f++)
		LD(ids[f]);
	return 0; /* the caller patches */
}

/* the gather's identifier patch: six big-endian bytes at data + offsets[i] + 8 */
uint32_t airs_dev_patch_ids_at(struct airs_dev_engine *e, void *data, const uint64_t *offsets, const uint64_t *ids,
			       uint64_t n)
{
	uint64_t i;
	int b;

	(void)e;
	for (i = 0; i < n; i++)
		for (b = 0; b < 6; b++)
			((uint8_t *)data)[offsets[i] + 8u + (uint64_t)b] = (uint8_t)(ids[i] >> (8 * (5 - b)));
	return 0;
}
