/*
 * ragged_plan_fuzz.c -- TEST ONLY: the ragged-piece planner of
 * cmp_gpu_compress_image (cmp_image_piece_next, cmp_image_ragged_blocks in
 * csrc/cmp_image_plan.c) under ASan + UBSan, linked with that file alone.
 *
 * Random lists of frame sizes with refused frames sprinkled in, budgets from
 * less than one frame's worth upward, keep thresholds from 0 to huge.  Checked:
 * every frame lies in exactly one piece and the pieces are in order; REFUSED
 * and RUN pieces are exactly what cmp_image_run_next gives, RUN pieces satisfy
 * the keep rule; no RAGGED piece holds a refused frame or a frame at which a
 * kept run starts, and one ends only where a rule says so; the budget and the
 * count limit are kept except by single-frame pieces; in a piece's block table
 * (frame, s) stands after (frame, s - 1) and every (frame, segment) appears
 * exactly once, in the order (segment, then frame).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cmp_image_plan.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;

static uint32_t rnd(void)
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return (uint32_t)(rng_state >> 16);
}

#define CHECK(c)                                                                  \
	do {                                                                      \
		if (!(c)) {                                                       \
			fprintf(stderr, "ragged_plan_fuzz: %s (line %d)\n", #c, __LINE__); \
			exit(1);                                                  \
		}                                                                 \
	} while (0)

/* a stand-in for cmp_compress_bound: 0 for a frame that is refused (equal
 * frames are refused alike: odd sizes and 0) */
static uint32_t bound_of(uint32_t fb)
{
	return (!fb || (fb & 1u)) ? 0u : 26u + 3u * fb;
}

static int kept(const uint32_t *fb, const uint32_t *bound, uint64_t n, uint64_t budget, uint64_t keep, uint64_t f,
		struct cmp_image_run *r)
{
	cmp_image_run_next(fb, n, budget, cmp_image_run_row(fb[f], bound[f]), 0, f, r);
	return bound[f] && r->count >= 2 && (uint64_t)r->count * fb[f] >= keep;
}

static void check_blocks(const uint32_t *segs, uint32_t count)
{
	uint32_t *active = malloc((size_t)(count ? count : 1u) * sizeof(*active));
	uint32_t *next = calloc(count ? count : 1u, sizeof(*next));
	const uint64_t total = cmp_image_ragged_blocks(segs, count, NULL, NULL);
	struct cmp_image_block *b = malloc((size_t)(total ? total : 1u) * sizeof(*b));
	uint64_t i, sum = 0;
	uint32_t j;

	CHECK(active && next && b);
	for (j = 0; j < count; j++)
		sum += segs[j];
	CHECK(total == sum);
	CHECK(cmp_image_ragged_blocks(segs, count, active, b) == total);
	for (i = 0; i < total; i++) {
		CHECK(b[i].frame < count);
		/* ascending segments per frame, none twice, none missing */
		CHECK(b[i].seg == next[b[i].frame]);
		CHECK(b[i].seg < segs[b[i].frame]);
		next[b[i].frame]++;
		/* (segment, then frame) */
		if (i)
			CHECK(b[i].seg > b[i - 1].seg || (b[i].seg == b[i - 1].seg && b[i].frame > b[i - 1].frame));
	}
	for (j = 0; j < count; j++)
		CHECK(next[j] == segs[j]);
	free(active);
	free(next);
	free(b);
}

static void one_case(uint32_t round)
{
	const uint64_t n = 1u + rnd() % (round % 7u == 0u ? 400u : 60u);
	uint32_t *fb = malloc((size_t)n * sizeof(*fb)), *bound = malloc((size_t)n * sizeof(*bound));
	uint32_t *segs = malloc((size_t)n * sizeof(*segs));
	const uint32_t seg = 1u + rnd() % 64u;
	uint64_t budget, keep, f, i;
	uint32_t max_frames, limit;
	struct cmp_image_piece p;
	struct cmp_image_run r;

	CHECK(fb && bound && segs);
	for (i = 0; i < n; i++) {
		const uint32_t w = rnd() % 16u;

		if (i && w < 6u)
			fb[i] = fb[i - 1]; /* a run */
		else if (w < 8u)
			fb[i] = rnd() % 3u ? 2u * (rnd() % 40u) + 1u : 0u; /* refused */
		else
			fb[i] = 2u * (1u + rnd() % (w < 12u ? 8u : 3000u));
		bound[i] = bound_of(fb[i]);
	}
	switch (rnd() % 5u) {
	case 0:
		budget = 0; /* the default */
		break;
	case 1:
		budget = 1u + rnd() % 64u; /* less than a frame's worth */
		break;
	default:
		budget = 1u + rnd() % 60000u;
		break;
	}
	switch (rnd() % 5u) {
	case 0:
		keep = 0;
		break;
	case 1:
		keep = UINT64_MAX;
		break;
	case 2:
		keep = (uint64_t)CMP_IMAGE_RAGGED_KEEP;
		break;
	default:
		keep = rnd() % 20000u;
		break;
	}
	max_frames = rnd() % 4u ? 0u : 1u + rnd() % 9u;
	limit = max_frames ? max_frames : CMP_IMAGE_RAGGED_FRAMES;
	for (f = 0; f < n; f += p.count) {
		const uint64_t b = budget ? budget : CMP_IMAGE_CHUNK_DEFAULT;

		memset(&p, 0xEE, sizeof(p));
		cmp_image_piece_next(fb, bound, n, budget, keep, max_frames, f, &p);
		CHECK(p.first == f && p.count >= 1 && f + p.count <= n);
		if (p.kind == CMP_IMAGE_PIECE_REFUSED || p.kind == CMP_IMAGE_PIECE_RUN) {
			const int k = kept(fb, bound, n, budget, keep, f, &r);

			CHECK(r.count == p.count);
			CHECK((p.kind == CMP_IMAGE_PIECE_REFUSED) == !bound[f]);
			CHECK(p.kind == CMP_IMAGE_PIECE_REFUSED || k);
			for (i = 0; i < p.count; i++)
				CHECK(fb[f + i] == fb[f]);
		} else {
			uint64_t sum = 0;

			CHECK(p.kind == CMP_IMAGE_PIECE_RAGGED);
			CHECK(!kept(fb, bound, n, budget, keep, f, &r) && bound[f]);
			for (i = 0; i < p.count; i++) {
				CHECK(bound[f + i]);
				CHECK(!kept(fb, bound, n, budget, keep, f + i, &r));
				sum += cmp_image_run_row(fb[f + i], bound[f + i]);
				segs[i] = (fb[f + i] / 2u + seg - 1u) / seg;
			}
			CHECK(p.count == 1 || (sum <= b && p.count <= limit));
			/* it ends where a rule says so */
			if (f + p.count < n) {
				const uint64_t g = f + p.count;

				CHECK(!bound[g] || kept(fb, bound, n, budget, keep, g, &r) || p.count == limit ||
				      sum + cmp_image_run_row(fb[g], bound[g]) > b);
			}
			check_blocks(segs, p.count);
			/* a pass group: some frames belong to the other launch */
			for (i = 0; i < p.count; i++)
				segs[i] = rnd() % 3u ? segs[i] : 0u;
			check_blocks(segs, p.count);
		}
	}
	CHECK(f == n);
	free(fb);
	free(bound);
	free(segs);
}

int main(void)
{
	uint32_t round;

	for (round = 0; round < 20000u; round++)
		one_case(round);
	printf("ragged_plan_fuzz: OK\n");
	return 0;
}
