/* cmp_pass.h -- what the cmp.h engine (cmp_host.c) and the batch planner
 * behind cmp_gpu_compress (cmp_batch.c) share: the pass a frame takes, the
 * steps of the context state machine that resolve it, the frame size bounds,
 * the launch builder.  Private to those two files; the functions are defined
 * and described in cmp_host.c and hidden from the library's exports. */
#ifndef CMP_PASS_H
#define CMP_PASS_H

#include "cmp.h"
#include "cmp_errors.h"
#include "cmp_gpu.h"
#include "airs_dev.h"

#define ERRV(name) ((uint32_t)0u - (uint32_t)CMP_ERR_##name)
#define CTX_MAGIC 34021395u      /* reference lib/compress/cmp.c:23 */
#define EXT_HDR_SIZE 6u          /* reference lib/common/header_private.h:35-39 */
#define HDR_MAX_SIZE (CMP_HDR_SIZE + EXT_HDR_SIZE)

static inline unsigned is_err(uint32_t v)
{
	return v > ERRV(MAX_CODE);
}

/* the pass a frame will use, resolved from the context (cmp.c:228-248) */
struct pass {
	uint32_t pre, enc, par, outlier_param, outlier;
	uint32_t model_mode;
	uint32_t hdr_bytes;
	uint8_t seq; /* a byte, as in the context and the header (walk_upload reads it at a stride) */
};

/* a batch's frames: bytes of a sample (2 or 4), samples of a frame, frames, u16 samples */
struct batch_shape {
	uint32_t bytes, n, total, is_unsigned;
};

enum { SLOT_SRC = 0, SLOT_DST, SLOT_MODEL, SLOT_STATUS, SLOT_CK, SLOT_IDS, SLOT_G, SLOT_AUX, SLOT_FL, SLOT_SIZES, SLOT_MSAVE };
/* a one-launch batch path's answer when it does not apply (nothing launched):
 * neither 0 nor an error value */
#define WALK_NO 1u

#pragma GCC visibility push(hidden)
uint64_t next_identifier(void);
int model_needed(const struct cmp_params *p);
int work_buf_state(const struct cmp_params *p);
uint32_t ctx_reset(struct cmp_context *ctx, uint32_t *draws);
uint32_t engine_prologue(struct cmp_context *ctx, void *dst, uint32_t cap, uint32_t n, struct pass *p, uint32_t *draws);
uint32_t fallback_prologue(struct cmp_context *ctx, void *dst, uint32_t raw, uint32_t n, struct pass *p, uint32_t *draws);
uint64_t payload_bound(uint32_t size);
uint64_t frame_worst(uint32_t n);
uint32_t launch_cap(uint32_t cap, uint32_t n);
uint64_t model_fail_bit(uint32_t cap, uint32_t n);
uint32_t raw_frame_size(const struct cmp_context *ctx, uint32_t n);
int size_field_can_overflow(const struct cmp_params *P, uint32_t n, uint32_t flags);
void launch_fill(struct airs_launch *L, const struct cmp_gpu_batch *b, const struct batch_shape *sh,
		 const struct cmp_context *ctx, const struct pass *p, uint32_t cap);
#pragma GCC visibility pop

#endif /* CMP_PASS_H */
