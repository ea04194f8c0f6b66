/* airs_rcp.h -- unsigned division by a launch constant as one multiply.
 *
 * The Rice kernel (enc_rice.hip) turns its block index d into (segment in
 * frame, launch frame) = (d / nfr, d % nfr), and for AUTO p into (p / spf,
 * p % spf).  The divisor is the same for the whole launch, so the host makes
 * its reciprocal once (KArgs.nfr_rcp, KArgs.spf_rcp) and every workgroup
 * multiplies.  Plain C: the host code, the kernels and
 * a stand-alone test program (tests/test_rice_rcp.py) include this file.
 *
 * Round-up method: m = ceil(2^32 / n) = (2^32 + e) / n with 0 <= e < n, and
 *   mulhi(d, m) = floor(d m / 2^32) = floor(d / n + d e / (n 2^32)).
 * With d = q n + r (r <= n - 1) the floor stays q while the error term is
 * below 1 / n, i.e. while d e < 2^32.  Since e <= n - 1,
 *
 *   the quotient is exact for every d with d n < 2^32, that is d < 2^32 / n
 *
 * (for a power of two e = 0 and it is exact for every d; the bound above is
 * kept for every n all the same).  n = 1 would need m = 2^32: the multiply
 * form passes d through instead, one scalar select in the kernel.
 *
 * airs_rcp_u32(n, count) returns 0 when some d < count lies past the bound
 * (or n = 0): the caller then divides, in the kernel with airs_udiv_slow (no
 * launch of the tests or the benchmark comes near the bound: 2^32 / nfr blocks).
 */
#ifndef AIRS_RCP_H
#define AIRS_RCP_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AIRS_RCP_FN static inline __host__ __device__
#else
#define AIRS_RCP_FN static inline
#endif

/* 1: a test build without reciprocals, every launch takes the kernel's
 * division branch (how that branch was run on the GPU) */
#ifndef AIRS_RCP_NONE
#define AIRS_RCP_NONE 0
#endif

/* the reciprocal of n for the dividends d < count, or 0 (divide instead) */
AIRS_RCP_FN uint32_t airs_rcp_u32(uint32_t n, uint64_t count)
{
	if (AIRS_RCP_NONE || n == 0u || (count && count - 1u > 0xFFFFFFFFull / n)) /* ((count - 1) n >= 2^32) */
		return 0u;
	if (n == 1u)
		return 0xFFFFFFFFu; /* not used: airs_rcp_div passes d through */
	return (uint32_t)(((1ull << 32) + n - 1u) / n);
}

/* d / n by the reciprocal rcp = airs_rcp_u32(n, count) != 0, for d < count */
AIRS_RCP_FN uint32_t airs_rcp_div(uint32_t d, uint32_t n, uint32_t rcp)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const uint32_t q = __umulhi(d, rcp);
#else
	const uint32_t q = (uint32_t)(((uint64_t)d * rcp) >> 32);
#endif
	return n == 1u ? d : q;
}

/* d / n (n != 0) by shift and subtract, exact for every d: integer ALU only
 * (on the GPU the `/` operator takes a floating-point reciprocal and a dozen
 * dependent instructions in line; this loop is a branch the kernel skips) */
AIRS_RCP_FN uint32_t airs_udiv_slow(uint32_t d, uint32_t n)
{
	uint32_t q = 0u, r = 0u;
	if (n > 0x80000000u) /* (r << 1 below would not fit) */
		return d >= n ? 1u : 0u;
#if defined(__clang__)
#pragma nounroll
#endif
	for (int i = 31; i >= 0; i--) {
		r = (r << 1) | ((d >> i) & 1u);
		if (r >= n) {
			r -= n;
			q |= 1u << i;
		}
	}
	return q;
}

#endif
