/*
 * img_copy.h -- what the byte-phase copies of the image calls share
 * (decode_image.hip, encode_image.hip): the workgroup's tile, the 16-byte
 * fetch at any alignment and the 16-bit byte swap.
 */
#ifndef AIRS_IMG_COPY_H
#define AIRS_IMG_COPY_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace airsimg {

#define IMG_WG 256u
#define IMG_LINES 4u // 16-byte lines per lane
#define IMG_TILE (IMG_WG * IMG_LINES * 16u)

// The 16 bytes at s (any alignment, s < end) from the two aligned lines around
// them.  The second line is requested only when it holds a byte below end, so
// no load leaves the aligned hull of the bytes the caller owns; what it would
// have held reads as zero.  The phase is the same for a whole workgroup (one
// frame), so the switch is a uniform branch.
__device__ __forceinline__ uint4 img_fetch16(const uint8_t *s, const uint8_t *end)
{
	const uintptr_t base = (uintptr_t)s & ~(uintptr_t)15u;
	const uint32_t p = (uint32_t)((uintptr_t)s & 15u), bs = p & 3u;
	const uint4 lo = *reinterpret_cast<const uint4 *>(base);
	uint4 hi = make_uint4(0u, 0u, 0u, 0u);
	if (p && base + 16u < (uintptr_t)end)
		hi = *reinterpret_cast<const uint4 *>(base + 16u);
#define IMG_AB(h, l) __builtin_amdgcn_alignbyte(h, l, bs)
	switch (p >> 2) {
	case 0:
		return make_uint4(IMG_AB(lo.y, lo.x), IMG_AB(lo.z, lo.y), IMG_AB(lo.w, lo.z), IMG_AB(hi.x, lo.w));
	case 1:
		return make_uint4(IMG_AB(lo.z, lo.y), IMG_AB(lo.w, lo.z), IMG_AB(hi.x, lo.w), IMG_AB(hi.y, hi.x));
	case 2:
		return make_uint4(IMG_AB(lo.w, lo.z), IMG_AB(hi.x, lo.w), IMG_AB(hi.y, hi.x), IMG_AB(hi.z, hi.y));
	default:
		return make_uint4(IMG_AB(hi.x, lo.w), IMG_AB(hi.y, hi.x), IMG_AB(hi.z, hi.y), IMG_AB(hi.w, hi.z));
	}
#undef IMG_AB
}

// the first r (< 16) bytes of v, the rest zero
__device__ __forceinline__ uint4 img_keep(uint4 v, uint32_t r)
{
	uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		const uint32_t keep = r > 4u * k ? min(r - 4u * k, 4u) : 0u;
		w[k] = keep == 4u ? w[k] : w[k] & ((1u << (8u * keep)) - 1u);
	}
	return make_uint4(w[0], w[1], w[2], w[3]);
}

// two 16-bit samples in a word, each byte-swapped
__device__ __forceinline__ uint32_t img_swap16x2(uint32_t v)
{
	return __builtin_amdgcn_perm(v, v, 0x02030001u);
}

} // namespace airsimg

#endif /* AIRS_IMG_COPY_H */
