/*
 * image_plan_fuzz.c -- cmp_gpu_frame_table and cmp_image_plan_next
 * (airs-compression_amd/csrc/cmp_image_plan.c) under ASan + UBSan, stand-alone
 * (tests/test_image_plan_sanitize.py compiles and runs it; no device, no
 * Python in the sanitized process).
 *
 * The table walker gets random and adversarial images in heap blocks of their
 * exact size, so a read past the image is a sanitizer report, and is checked
 * against a walk written here.  The planner gets random size lists at budgets
 * from one frame's worth upward; every frame must lie in exactly one chunk,
 * the chunks in order, the budget kept except by single-frame chunks, no chunk
 * above 65535 frames, and every row wide enough for its frames.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cmp_gpu.h"
#include "cmp_image_plan.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;

static uint64_t rnd(void)
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return rng_state;
}

#define FAIL(...)                                     \
	do {                                          \
		fprintf(stderr, "FAIL: " __VA_ARGS__); \
		fprintf(stderr, "\n");                \
		exit(1);                              \
	} while (0)

static void put24(uint8_t *p, uint32_t v)
{
	p[0] = (uint8_t)(v >> 16);
	p[1] = (uint8_t)(v >> 8);
	p[2] = (uint8_t)v;
}

static void check_table(const uint8_t *img, uint64_t size, const char *what)
{
	uint64_t want[4096], nwant = 0, pos = 0, bad = UINT64_MAX, got_bad = 7, n, i, room;
	uint64_t *offs;

	while (pos < size) {
		uint32_t fs;

		if (size - pos < 16) {
			bad = pos;
			break;
		}
		fs = (uint32_t)img[pos + 2] << 16 | (uint32_t)img[pos + 3] << 8 | img[pos + 4];
		if (fs < 16 || fs > size - pos) {
			bad = pos;
			break;
		}
		if (nwant < 4096)
			want[nwant] = pos;
		nwant++;
		pos += fs;
	}
	/* count only */
	n = cmp_gpu_frame_table(img, size, NULL, 0, &got_bad);
	if (n != nwant || got_bad != bad)
		FAIL("%s: count %llu (want %llu), bad_at %llu (want %llu)", what, (unsigned long long)n,
		     (unsigned long long)nwant, (unsigned long long)got_bad, (unsigned long long)bad);
	if (cmp_gpu_frame_table(img, size, NULL, UINT64_MAX, NULL) != nwant)
		FAIL("%s: count without bad_at", what);
	/* a table of exactly `room` entries on the heap: one write too many is a report */
	for (room = 0; room <= nwant + 1 && room <= 4096; room += (nwant / 3) + 1) {
		offs = malloc(room ? room * 8 : 1);
		if (!offs)
			FAIL("malloc");
		n = cmp_gpu_frame_table(img, size, offs, room, &got_bad);
		if (n != nwant || got_bad != bad)
			FAIL("%s: room %llu", what, (unsigned long long)room);
		for (i = 0; i < room && i < nwant; i++)
			if (offs[i] != want[i])
				FAIL("%s: offset %llu", what, (unsigned long long)i);
		free(offs);
	}
}

static void fuzz_table(void)
{
	int round;

	check_table(NULL, 0, "empty");
	for (round = 0; round < 3000; round++) {
		const uint64_t size = rnd() % 700;
		uint8_t *img = malloc(size ? size : 1);
		uint64_t pos = 0;
		const int kind = (int)(rnd() % 4);

		if (!img)
			FAIL("malloc");
		for (pos = 0; pos < size; pos++)
			img[pos] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? 0xFF : 0;
		if (kind >= 2) { /* well-formed frames, then (kind 3) one damaged size field */
			for (pos = 0; size - pos >= 16;) {
				uint32_t fs = 16 + (uint32_t)(rnd() % 90);

				if (fs > size - pos || size - pos - fs < 16)
					fs = (uint32_t)(size - pos);
				put24(img + pos + 2, fs);
				pos += fs;
			}
			if (kind == 3 && size >= 16) {
				const uint32_t v[6] = {0, 15, 16, 0xFFFFFF, (uint32_t)size, (uint32_t)size + 1};

				put24(img + 2, v[rnd() % 6]);
			}
		}
		check_table(img, size, "random");
		free(img);
	}
}

static uint32_t up16(uint32_t v)
{
	return (v + 15u) & ~15u;
}

static void check_plan(const uint32_t *fr, uint64_t n, uint64_t budget, const char *what)
{
	uint64_t first = 0, f;

	while (first < n) {
		struct cmp_image_chunk c;
		const uint64_t eff = budget ? budget : CMP_IMAGE_CHUNK_DEFAULT;

		memset(&c, 0xEE, sizeof(c));
		cmp_image_plan_next(fr, n, budget, first, &c);
		/* chunks follow each other, so every frame is in exactly one */
		if (c.first != first || !c.count || c.count > CMP_IMAGE_CHUNK_FRAMES || c.count > n - first)
			FAIL("%s: chunk at %llu: first %llu count %u", what, (unsigned long long)first,
			     (unsigned long long)c.first, c.count);
		if (c.count > 1 && (uint64_t)c.count * ((uint64_t)c.src_cap + c.dst_stride) > eff)
			FAIL("%s: chunk at %llu over the budget", what, (unsigned long long)first);
		if ((c.src_cap & 15u) || c.src_cap < CMP_IMAGE_ROW_MIN || !c.dst_samples ||
		    c.dst_stride != up16(2u * c.dst_samples))
			FAIL("%s: chunk at %llu: row widths", what, (unsigned long long)first);
		for (f = first; f < first + c.count; f++)
			if (fr[2 * f] > c.src_cap || fr[2 * f + 1] > c.dst_samples)
				FAIL("%s: frame %llu does not fit its row", what, (unsigned long long)f);
		if (first && fr[2 * (first - 1) + 1] > c.dst_samples)
			FAIL("%s: chunk at %llu cannot hold the model that comes in", what, (unsigned long long)first);
		/* greedy: the next frame would not have fitted */
		if (first + c.count < n && c.count < CMP_IMAGE_CHUNK_FRAMES) {
			const uint32_t cap = up16(fr[2 * (first + c.count)]) > c.src_cap ? up16(fr[2 * (first + c.count)])
										       : c.src_cap;
			const uint32_t nn = fr[2 * (first + c.count) + 1] > c.dst_samples ? fr[2 * (first + c.count) + 1]
											  : c.dst_samples;

			if (((uint64_t)c.count + 1u) * ((uint64_t)cap + up16(2u * nn)) <= eff)
				FAIL("%s: chunk at %llu stops early", what, (unsigned long long)first);
		}
		first += c.count;
	}
}

static void fuzz_plan(void)
{
	int round;
	uint64_t i;

	for (round = 0; round < 400; round++) {
		const uint64_t n = 1 + rnd() % (round % 50 == 0 ? 140000 : 300);
		uint32_t *fr = malloc(n * 8);
		uint64_t one = 0, budget;
		const int shape = (int)(rnd() % 4);

		if (!fr)
			FAIL("malloc");
		for (i = 0; i < n; i++) {
			uint32_t cs = 16 + (uint32_t)(rnd() % (shape == 1 ? 40 : 5000)), ns = (uint32_t)(rnd() % 3000);

			if (shape == 2 && rnd() % 64 == 0) { /* one large frame next to small ones */
				cs = 0xFFFFFF;
				ns = 0x7FFFFF;
			}
			if (rnd() % 16 == 0) /* an unusable slice */
				cs = ns = 0;
			fr[2 * i] = cs;
			fr[2 * i + 1] = ns;
			if ((uint64_t)up16(cs) + up16(2u * ns) > one)
				one = (uint64_t)up16(cs) + up16(2u * ns);
		}
		/* from one frame's worth upward (and below it: single-frame chunks), and the default */
		check_plan(fr, n, 1, "budget 1");
		for (budget = one; budget < one * 2 * n && budget < (1ull << 40); budget = budget * 3 + 1)
			check_plan(fr, n, budget, "budget from one frame up");
		check_plan(fr, n, 0, "default budget");
		check_plan(fr, n, UINT64_MAX, "no budget");
		free(fr);
	}
}

int main(void)
{
	fuzz_table();
	fuzz_plan();
	printf("image_plan_fuzz: OK\n");
	return 0;
}
