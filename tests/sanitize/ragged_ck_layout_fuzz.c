/*
 * ragged_ck_layout_fuzz.c -- TEST ONLY: the layout of the ragged checksum's
 * products (cmp_image_ck_region, cmp_image_ck_layout in
 * csrc/cmp_image_plan.c) under ASan + UBSan, linked with that file alone.
 *
 * Pseudo-random tables of frame sizes, both sample widths.  Checked: every
 * offset is a multiple of 16 (of 64, in fact); the regions stand in table
 * order and do not overlap; a region holds at least the frame's products
 * (16 bytes per stripe of 8 samples) and takes at most 2 n + 128 bytes; the
 * total is the sum of the regions, which is what the caller allocates; the
 * counting call (NULL tables) answers what the filling call answers; the
 * product workgroups cover every round quad of every frame exactly once, in
 * table order, and name no quad past a frame's own; the chain kernel's slot
 * order is the table's, so the slots are a permutation of the frames by
 * construction (slot j = frame j: no table to check).  Frame counts of 1 and of
 * 2^20 and sample counts of 1 and of the largest a 32-bit size holds do not
 * overflow.
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

#define CHECK(c)                                                                       \
	do {                                                                           \
		if (!(c)) {                                                            \
			fprintf(stderr, "ragged_ck_layout_fuzz: %s (line %d)\n", #c, __LINE__); \
			exit(1);                                                       \
		}                                                                      \
	} while (0)

static void check_table(const uint32_t *fb, uint32_t sb, uint32_t count)
{
	uint64_t nb0 = 0, nb = 0, total0, total, sum = 0, b = 0;
	uint64_t *off = malloc((size_t)count * sizeof(*off));
	struct cmp_image_ck_block *blk;
	uint32_t j;

	CHECK(off);
	total0 = cmp_image_ck_layout(fb, sb, count, NULL, NULL, &nb0);
	blk = malloc((size_t)(nb0 ? nb0 : 1u) * sizeof(*blk));
	CHECK(blk);
	total = cmp_image_ck_layout(fb, sb, count, off, blk, &nb);
	CHECK(total == total0 && nb == nb0);
	CHECK(cmp_image_ck_layout(fb, sb, count, off, NULL, NULL) == total);
	for (j = 0; j < count; j++) {
		const uint32_t n = fb[j] / sb;
		const uint64_t region = cmp_image_ck_region(n);
		const uint64_t quads = region / CMP_IMAGE_CK_QUAD;
		uint64_t q;

		CHECK(off[j] % 16u == 0 && off[j] % CMP_IMAGE_CK_QUAD == 0);
		CHECK(off[j] == sum); /* back to back in table order: no overlap, no hole */
		CHECK(region % CMP_IMAGE_CK_QUAD == 0);
		CHECK(region >= (uint64_t)(n / 8u) * 16u);
		CHECK(region <= 2ull * n + 128u);
		CHECK(n >= 8u || region == 0);
		sum += region;
		CHECK(sum <= total);
		/* the frame's product workgroups: 256 quads each, ascending, the last one partial */
		for (q = 0; q < quads; q += CMP_IMAGE_CK_BLOCK_QUADS, b++) {
			CHECK(b < nb);
			CHECK(blk[b].frame == j);
			CHECK((uint64_t)blk[b].qb * CMP_IMAGE_CK_BLOCK_QUADS == q);
		}
	}
	CHECK(sum == total && b == nb);
	free(off);
	free(blk);
}

int main(void)
{
	static const uint32_t edge_n[] = {1, 2, 7, 8, 9, 15, 16, 31, 32, 33, 8191, 8192, 8193, 8200, 65536, 65538};
	uint32_t *fb = malloc((size_t)(1u << 20) * sizeof(*fb));
	uint32_t round, j, sb;

	CHECK(fb);
	/* one frame, every edge size */
	for (sb = 2; sb <= 4; sb += 2)
		for (j = 0; j < sizeof(edge_n) / sizeof(edge_n[0]); j++) {
			fb[0] = edge_n[j] * sb;
			check_table(fb, sb, 1);
		}
	/* the largest frames a 32-bit size holds: the sums need 64 bits */
	for (sb = 2; sb <= 4; sb += 2) {
		for (j = 0; j < 4; j++)
			fb[j] = 0xFFFFFFFFu / sb * sb;
		check_table(fb, sb, 4);
		fb[0] = 0xFFFFFFFFu / sb * sb;
		check_table(fb, sb, 1);
	}
	/* 2^20 frames: of one sample each, then of mixed small sizes */
	for (j = 0; j < 1u << 20; j++)
		fb[j] = 2;
	check_table(fb, 2, 1u << 20);
	for (j = 0; j < 1u << 20; j++)
		fb[j] = 4u * (1u + rnd() % 3000u);
	check_table(fb, 4, 1u << 20);
	/* random tables: mostly small frames, some around the workgroup edge, a few of millions of samples */
	for (round = 0; round < 3000; round++) {
		const uint32_t count = 1u + rnd() % 200u;

		sb = (rnd() & 1u) ? 2u : 4u;
		for (j = 0; j < count; j++) {
			const uint32_t kind = rnd() % 16u;
			uint32_t n;

			if (kind < 8u)
				n = 1u + rnd() % 100u;
			else if (kind < 12u)
				n = 8192u * (1u + rnd() % 3u) - 40u + rnd() % 80u;
			else if (kind < 15u)
				n = 1u + rnd() % 100000u;
			else
				n = 1u + rnd() % (4u << 20);
			fb[j] = n * sb;
		}
		check_table(fb, sb, count);
	}
	free(fb);
	printf("ragged_ck_layout_fuzz: OK\n");
	return 0;
}
