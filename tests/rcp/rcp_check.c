/* rcp_check.c -- exhaustive check of csrc/airs_rcp.h on the CPU
 * (tests/test_rice_rcp.py builds it plain and with ASan + UBSan).
 *
 *   rcp_check nfr LO HI   every divisor n in [LO, HI] as a frame count
 *   rcp_check spf LO HI   ... as the segments of a frame
 *   rcp_check bound       airs_rcp_u32's answers on both sides of the bound
 *   rcp_check slow        airs_udiv_slow against `/`
 *
 * For every n the multiply form airs_rcp_div(d, n, airs_rcp_u32(n, count)) is
 * compared with d / n, and d - q n with d % n, for every d below the bound
 * documented in airs_rcp.h (d n < 2^32), or below 2^22 where the bound is
 * larger.  Prints the number of dividends checked; exit status 1 on the first
 * mismatch.
 */
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "airs_rcp.h"

#define DCAP (1u << 22)

static uint64_t bound_of(uint32_t n) /* the first d past the bound: ceil(2^32 / n) */
{
	return ((1ull << 32) + n - 1u) / n;
}

static int sweep(uint32_t lo, uint32_t hi)
{
	uint64_t checked = 0;
	for (uint32_t n = lo; n <= hi; n++) {
		const uint64_t b = bound_of(n);
		const uint32_t count = (uint32_t)(b < DCAP ? b : DCAP);
		const uint32_t rcp = airs_rcp_u32(n, count);
		if (rcp == 0u) {
			printf("n %" PRIu32 ": no reciprocal for %" PRIu32 " dividends\n", n, count);
			return 1;
		}
		for (uint32_t d = 0; d < count; d++) {
			const uint32_t q = airs_rcp_div(d, n, rcp);
			if (q != d / n || d - q * n != d % n) {
				printf("n %" PRIu32 " d %" PRIu32 ": %" PRIu32 " != %" PRIu32 "\n", n, d, q, d / n);
				return 1;
			}
		}
		checked += count;
	}
	printf("checked %" PRIu64 "\n", checked);
	return 0;
}

static int bound(void)
{
	static const uint32_t ns[] = {1u, 2u, 3u, 5u, 7u, 8u, 9u, 16u, 24u, 255u, 511u, 1000u, 4096u, 65535u, 65536u,
				      65537u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
	for (size_t i = 0; i < sizeof(ns) / sizeof(ns[0]); i++) {
		const uint32_t n = ns[i];
		const uint64_t last = bound_of(n); /* the largest count whose dividends all have d n < 2^32 */
		if (airs_rcp_u32(n, last) == 0u || airs_rcp_u32(n, 1u) == 0u) {
			printf("n %" PRIu32 ": 0 inside the bound\n", n);
			return 1;
		}
		if (airs_rcp_u32(n, last + 1u) != 0u || airs_rcp_u32(n, UINT64_MAX / n) != 0u) {
			printf("n %" PRIu32 ": a reciprocal past the bound\n", n);
			return 1;
		}
		/* the dividends next to the bound itself */
		const uint32_t rcp = airs_rcp_u32(n, last);
		for (uint64_t d = last > 4096u ? last - 4096u : 0u; d < last; d++)
			if (airs_rcp_div((uint32_t)d, n, rcp) != (uint32_t)d / n) {
				printf("n %" PRIu32 " d %" PRIu64 " below the bound: wrong quotient\n", n, d);
				return 1;
			}
	}
	if (airs_rcp_u32(0u, 1u) != 0u) {
		printf("n 0: a reciprocal\n");
		return 1;
	}
	printf("bound ok\n");
	return 0;
}

static int slow(void)
{
	uint32_t x = 0x9E3779B9u;
	uint64_t checked = 0;
	for (uint32_t i = 0; i < 200000u; i++) {
		x = x * 1664525u + 1013904223u;
		const uint32_t d = x >> (i % 29u);
		x = x * 1664525u + 1013904223u;
		uint32_t n = x >> (i % 31u);
		n = n ? n : 1u;
		if (airs_udiv_slow(d, n) != d / n) {
			printf("slow: %" PRIu32 " / %" PRIu32 "\n", d, n);
			return 1;
		}
		checked++;
	}
	static const uint32_t edge[] = {0u, 1u, 2u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu};
	for (size_t i = 0; i < 8; i++)
		for (size_t j = 1; j < 8; j++, checked++)
			if (airs_udiv_slow(edge[i], edge[j]) != edge[i] / edge[j]) {
				printf("slow: %" PRIu32 " / %" PRIu32 "\n", edge[i], edge[j]);
				return 1;
			}
	printf("checked %" PRIu64 "\n", checked);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 4 && (!strcmp(argv[1], "nfr") || !strcmp(argv[1], "spf")))
		return sweep((uint32_t)strtoul(argv[2], NULL, 10), (uint32_t)strtoul(argv[3], NULL, 10));
	if (argc == 2 && !strcmp(argv[1], "bound"))
		return bound();
	if (argc == 2 && !strcmp(argv[1], "slow"))
		return slow();
	fprintf(stderr, "usage: rcp_check nfr|spf LO HI | bound | slow\n");
	return 2;
}
