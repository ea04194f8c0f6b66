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

/* ---- ragged pieces (CMP_GPU_OPT_IMAGE_RAGGED) ---- */

/* The built-in keep threshold (option value 1): a run of equal frames with
 * fewer bytes of samples than this joins a ragged piece instead of taking a
 * batch launch, a scan and an emit of its own.  Not below 1 MiB: a run's fixed
 * cost (about 12 us) is more than ten times what even a
 * twice-slower kernel loses on 1 MiB of samples.  DESIGN.md 3.4.5 has the
 * table that decides the value. */
#define CMP_IMAGE_RAGGED_KEEP (1u << 20)
#define CMP_IMAGE_RAGGED_FRAMES (1u << 20) /* frames per ragged piece at most: the slice of the copies' grids */

enum cmp_image_piece_kind {
	CMP_IMAGE_PIECE_REFUSED = 0, /* a run of frames the loop's call refuses: the scan alone */
	CMP_IMAGE_PIECE_RUN = 1,     /* a run of equal frames kept on the batch path */
	CMP_IMAGE_PIECE_RAGGED = 2   /* frames of any sizes in one ragged launch per pass */
};

struct cmp_image_piece {
	uint64_t first;
	uint32_t count; /* >= 1 */
	uint32_t kind;  /* enum cmp_image_piece_kind */
};

/* The piece that starts at frame `first` < num_frames.  bound[f] is frame f's
 * capacity, 0 for a frame that is refused (equal frames are refused alike).
 * With R the run cmp_image_run_next cuts at `first` (row_bytes the
 * cmp_image_run_row of its frames, max_frames 0):
 *   REFUSED  bound[first] == 0: the piece is R;
 *   RUN      R has at least 2 frames and count * frame_bytes >= keep_bytes: R;
 *   RAGGED   otherwise the piece takes frame `first` and then following frames
 *            while the next frame is not refused, the run that would start at
 *            it is no kept RUN, the sum of cmp_image_run_row over the piece
 *            stays within `budget` (0: the default) and the count within
 *            max_frames (0, or anything above it: CMP_IMAGE_RAGGED_FRAMES). */
void cmp_image_piece_next(const uint32_t *frame_bytes, const uint32_t *bound, uint64_t num_frames, uint64_t budget,
			  uint64_t keep_bytes, uint32_t max_frames, uint64_t first, struct cmp_image_piece *piece);

/* one block of a ragged launch: segment `seg` of the piece's frame `frame` */
struct cmp_image_block {
	uint32_t frame, seg;
};

/* The blocks of one ragged launch, in dispatch order: segs[j] is the segment
 * count of the piece's frame j in this launch (0: the frame belongs to the
 * other pass).  Ordered by segment index, then frame: every frame's segment 0
 * in table order, then every frame's segment 1, and so on, so that (frame, s)
 * always stands after (frame, s - 1) and every (frame, segment) appears once.
 * `active` is scratch of `count` words.  Returns the number of blocks; with
 * blocks NULL it only counts (active may be NULL too). */
uint64_t cmp_image_ragged_blocks(const uint32_t *segs, uint32_t count, uint32_t *active,
				 struct cmp_image_block *blocks);

/* ---- the ragged checksum's products (CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM) ---- */

/* The XXH32 of a frame of n samples consumes n / 8 stripes of 16 bytes; the
 * product kernel writes them x P2 in round quads of 64 bytes (accumulator q's
 * four rounds at bytes 16 q of the quad), so a frame's region is its stripes
 * rounded up to a quad: at most 2 n + 48 bytes, nothing for n < 8. */
#define CMP_IMAGE_CK_QUAD 64u          /* bytes of one round quad */
#define CMP_IMAGE_CK_BLOCK_QUADS 256u  /* round quads one product workgroup forms */

/* one workgroup of the product kernel: round quads [256 qb, 256 qb + 256) of `frame` */
struct cmp_image_ck_block {
	uint32_t frame, qb;
};

/* bytes of the products of a frame of n samples (a multiple of 64) */
uint64_t cmp_image_ck_region(uint32_t n);

/* The products of a piece's `count` frames (frame j has frame_bytes[j] /
 * sample_bytes samples, at least 1) back to back in table order: off[j] is
 * frame j's byte offset (a multiple of 64), the regions do not overlap, the
 * return value is their sum, which the caller allocates.  blocks receives the
 * product workgroups, frame by frame (a frame under 8 samples has none), and
 * *num_blocks their number.  off and blocks may be NULL: it only counts.
 * The chain kernel takes the frames in table order: a wave of sixteen frames
 * lasts as long as its longest, whatever the order, and the waves of a piece
 * run side by side, so an order by size was not built. */
uint64_t cmp_image_ck_layout(const uint32_t *frame_bytes, uint32_t sample_bytes, uint32_t count, uint64_t *off,
			     struct cmp_image_ck_block *blocks, uint64_t *num_blocks);

#ifdef __cplusplus
}
#endif

#endif /* CMP_IMAGE_PLAN_H */
