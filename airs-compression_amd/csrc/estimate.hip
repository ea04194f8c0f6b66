/*
 * estimate.hip -- airs_dev_estimate (airs_dev.h): the exact payload bits of
 * every frame under many parameter sets, without coding anything
 * (cmp_gpu_estimate, include/cmp_gpu.h).
 *
 * A frame's payload is the sum over its samples of a codeword length, and the
 * length depends on the mapped residual and the coder alone
 * (cmp_encoder_encode_s16, reference lib/compress/encoder.c:303-378):
 *
 *   golomb(v)     v < cutoff ? k + 1 : k + 2 + (v - cutoff) / g
 *   UNCOMPRESSED  16
 *   GOLOMB_ZERO   m < outlier ? golomb(m + 1) : k + 17
 *   GOLOMB_MULTI  m < outlier ? golomb(m)
 *                             : golomb(outlier + lvl) + 2 (lvl + 1),
 *                 d = m - outlier, lvl = d < 4 ? 0 : floor(log2 d) / 2
 *
 * with m the zigzag of the 16-bit residual.  For g = 2^k the cutoff is g and
 * golomb(v) = k + 1 + (v >> k); GOLOMB_ZERO's outlier is then 17 g - 1, so its
 * length is k + 1 + min((m + 1) >> k, 16), three instructions a sample.
 *
 *   est_size_kernel    grid.x = slices * frames, 256 lanes.  A workgroup sizes
 *                      one slice (EST_SLICE samples: EST_SLICE / EST_CHUNK steps
 *                      of EST_CHUNK) of one frame under one GROUP of up to
 *                      EST_GROUP candidates, which it reads from its kernel
 *                      arguments (uniform, scalar loads).  Per step a lane
 *                      loads 16 samples, forms the mapped residual once per
 *                      preprocessing the group uses and adds every candidate's
 *                      lengths into that candidate's per-lane 32-bit
 *                      accumulator (LDS: a runtime loop over the candidates
 *                      keeps the kernel small).  Wave shuffle, LDS, then one
 *                      64-bit partial per (frame, slice, candidate) stored
 *                      to scratch.
 *   est_finish_kernel  one wave per frame, lane c candidate c: the sum of the
 *                      frame's partials into bits, the argmin into best.
 *
 * The finishing kernel follows the sizing launches in stream order: no
 * workgroup waits for another, nothing is counted or fenced.  IWT candidates
 * are sized as NONE over the coefficients, which the encoder's transform
 * (airs_dev_iwt) writes into scratch first.  The frames of a call are cut into
 * chunks so that the partials and the coefficients of a chunk stay bounded.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "airs_dev.h"
#include "airs_rcp.h"

namespace airsest {

#define E_GENERIC 1u
#define ERRV(c) ((uint32_t)0u - (uint32_t)(c))

#define EST_PT 16u                    // samples per lane and step
#define EST_CHUNK (256u * EST_PT)     // samples per workgroup and step
#define EST_SLICE (16u * EST_CHUNK)   // samples per workgroup
#define EST_GROUP 16u                 // candidates per launch (16 KiB of accumulators in LDS)
#define EST_PARTIAL_MAX (64ull << 20) // bytes of partials per chunk of frames
#define EST_IWT_MAX (256ull << 20)    // bytes of IWT coefficients per chunk of frames

#define PRE_NONE 0u
#define PRE_DIFF 1u
#define PRE_MODEL 3u

// one candidate in four words (the table stays in scalar registers): what =
// kind | pre << 2 | k << 4 | (g is a power of two) << 8 | col << 16, col the
// candidate's index in the call: its column of the partials.  The outlier is
// clamped to 65536 (no mapped value reaches it either way); rcp is
// airs_rcp_u32(g, 65537) and used for a g that is no power of two (not 1)
struct EstSlot {
	uint32_t what, cutoff, outlier, rcp;
	__host__ __device__ uint32_t kind() const { return what & 3u; }
	__host__ __device__ uint32_t pre() const { return (what >> 2) & 3u; }
	__host__ __device__ uint32_t k() const { return (what >> 4) & 15u; }
	__host__ __device__ bool p2() const { return (what >> 8) & 1u; }
	__host__ __device__ uint32_t col() const { return what >> 16; }
};

struct EstArgs {
	const uint8_t *src;
	uint64_t src_stride;
	const uint8_t *model;
	uint64_t model_stride;
	uint64_t *partial; // [frames of the chunk][slices][num_cand]
	uint32_t n, slices, num_cand;
	uint32_t count;    // slots in use
	uint32_t pre_mask; // bit p: a slot has preprocessing p
	EstSlot slot[EST_GROUP];
};

template <int W>
__device__ __forceinline__ uint32_t est_sample(const uint8_t *f, uint32_t i)
{
	return W == 2 ? (uint32_t)reinterpret_cast<const uint16_t *>(f)[i]
		      : reinterpret_cast<const uint32_t *>(f)[i] & 0xFFFFu;
}

// zigzag of the low 16 bits of r as a signed value: 0 .. 65535
__device__ __forceinline__ uint32_t est_map(uint32_t r)
{
	const int32_t d = (int32_t)(r << 16) >> 16;
	return ((uint32_t)d << 1) ^ (uint32_t)(d >> 31);
}

__device__ __forceinline__ uint32_t est_golomb(const EstSlot &c, uint32_t k, uint32_t v, bool p2)
{
	// every dividend is below 65537 (v <= 65536), where the reciprocal is exact
	// for every g (airs_rcp.h: airs_rcp_div for a g that is not 1); a wrapped
	// v - cutoff belongs to the other arm
	const uint32_t d = v - c.cutoff;
	const uint32_t q = p2 ? d >> k : __umulhi(d, c.rcp);
	return v < c.cutoff ? k + 1u : k + 2u + q;
}

// the lengths of NS mapped residuals under slot c, without what is the same
// for every sample (est_fixed_bits)
template <uint32_t NS>
__device__ __forceinline__ uint32_t est_lengths(const EstSlot &c, const uint32_t (&m)[NS])
{
	uint32_t s = 0u;
	const uint32_t kind = c.kind(), k = c.k();
	if (kind == AIRS_EST_ZERO_P2) {
#pragma unroll
		for (uint32_t j = 0; j < NS; j++)
			s += min((m[j] + 1u) >> k, 16u);
	} else if (kind == AIRS_EST_ZERO) {
#pragma unroll
		for (uint32_t j = 0; j < NS; j++)
			s += m[j] < c.outlier ? est_golomb(c, k, m[j] + 1u, false) : k + 17u;
	} else if (kind == AIRS_EST_MULTI) {
		const bool p2 = c.p2();
#pragma unroll
		for (uint32_t j = 0; j < NS; j++) {
			const bool esc = m[j] >= c.outlier;
			const uint32_t d = m[j] - c.outlier;
			const uint32_t lvl = (31u - (uint32_t)__clz((int)(d | 1u))) >> 1;
			s += est_golomb(c, k, esc ? c.outlier + lvl : m[j], p2) + (esc ? 2u * lvl + 2u : 0u);
		}
	}
	return s;
}

// what every sample of slot c costs on top of est_lengths
__device__ __forceinline__ uint32_t est_fixed_bits(const EstSlot &c)
{
	return c.kind() == AIRS_EST_RAW ? 16u : c.kind() == AIRS_EST_ZERO_P2 ? c.k() + 1u : 0u;
}

typedef __attribute__((address_space(3))) uint32_t est_lds_u32;

// NS samples x (the one before them in xp, their model in xm) into the lane's
// accumulators acc[c * 256]: the residual once per preprocessing of the
// group, then every candidate of that preprocessing (uniform branches)
template <uint32_t NS>
__device__ __forceinline__ void est_accumulate(const EstArgs &a, const uint32_t (&x)[NS], uint32_t xp,
					       const uint32_t (&xm)[NS], uint32_t *acc)
{
	for (uint32_t p = 0; p < 4u; p++) {
		if (!((a.pre_mask >> p) & 1u))
			continue;
		uint32_t m[NS];
		if (p == PRE_NONE) {
#pragma unroll
			for (uint32_t j = 0; j < NS; j++)
				m[j] = est_map(x[j]);
		} else if (p == PRE_DIFF) {
#pragma unroll
			for (uint32_t j = 0; j < NS; j++)
				m[j] = est_map(x[j] - (j ? x[(j + NS - 1u) % NS] : xp));
		} else {
#pragma unroll
			for (uint32_t j = 0; j < NS; j++)
				m[j] = est_map(x[j] - xm[j]);
		}
#pragma nounroll
		for (uint32_t c = 0; c < a.count; c++) {
			const EstSlot t = a.slot[c];
			if (t.pre() != p || t.kind() == AIRS_EST_RAW)
				continue;
			// the lane's own word: an add that returns nothing and is not waited for
			__hip_atomic_fetch_add(reinterpret_cast<est_lds_u32 *>((uintptr_t)(acc + c * 256u)),
					       est_lengths<NS>(t, m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		}
	}
}

// Three waves per SIMD (at most 168 VGPRs): the samples, the
// models and the mapped residuals of a step are 48 registers, and the sixteen
// lengths of a candidate are independent chains that hide the ALU's latency
// without help from other waves.  Capped at 128 registers the compiler spills.
template <int W>
__global__ __launch_bounds__(256) void est_size_kernel(const EstArgs a)
{
	// a 32-bit accumulator per candidate and lane (48 bits a sample at most,
	// EST_SLICE / 256 samples a lane); a wave's adds never share a bank
	__shared__ uint32_t s_acc[EST_GROUP][256];
	__shared__ uint32_t s_part[EST_GROUP][4];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t frame = blockIdx.x / a.slices, slice = blockIdx.x - frame * a.slices;
	const uint8_t *f = a.src + (uint64_t)frame * a.src_stride;
	const uint8_t *fm = a.model ? a.model + (uint64_t)frame * a.model_stride : nullptr;
	const bool need_m = (a.pre_mask >> PRE_MODEL) & 1u, need_p = (a.pre_mask >> PRE_DIFF) & 1u;
	const bool al = ((uintptr_t)f & 15u) == 0u, alm = ((uintptr_t)fm & 15u) == 0u;
	const uint32_t n = a.n, s0 = slice * EST_SLICE;
	const uint32_t send = n - s0 < EST_SLICE ? n : s0 + EST_SLICE; // s0 < n: slices = ceil(n / EST_SLICE)
	uint32_t *acc = &s_acc[0][tid];
	for (uint32_t c = 0; c < a.count; c++)
		acc[c * 256u] = 0u; // the lane's own words: no barrier before its adds
	// the step count is uniform: the shuffle below needs every lane of the wave
	for (uint32_t cb = s0; cb < send; cb += EST_CHUNK) {
		const uint32_t i = cb + tid * EST_PT;
		const bool whole = i < send && send - i >= EST_PT;
		uint32_t x[EST_PT], xm[EST_PT];
#pragma unroll
		for (uint32_t j = 0; j < EST_PT; j++)
			x[j] = xm[j] = 0u;
		if (whole) {
			if (al) {
				// 16 samples as W 16-byte loads, inside the frame
				const uint4 *q = reinterpret_cast<const uint4 *>(f + (size_t)i * W);
#pragma unroll
				for (uint32_t u = 0; u < (uint32_t)W; u++) {
					const uint4 r = q[u];
					const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
					for (uint32_t e = 0; e < 4u; e++) {
						if (W == 2) {
							x[8u * u + 2u * e] = w[e] & 0xFFFFu;
							x[8u * u + 2u * e + 1u] = w[e] >> 16;
						} else {
							x[4u * u + e] = w[e] & 0xFFFFu;
						}
					}
				}
			} else {
#pragma unroll
				for (uint32_t j = 0; j < EST_PT; j++)
					x[j] = est_sample<W>(f, i + j);
			}
			if (need_m) {
				if (alm) {
					const uint4 *q = reinterpret_cast<const uint4 *>(fm + (size_t)i * 2u);
#pragma unroll
					for (uint32_t u = 0; u < 2u; u++) {
						const uint4 r = q[u];
						const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
						for (uint32_t e = 0; e < 4u; e++) {
							xm[8u * u + 2u * e] = w[e] & 0xFFFFu;
							xm[8u * u + 2u * e + 1u] = w[e] >> 16;
						}
					}
				} else {
#pragma unroll
					for (uint32_t j = 0; j < EST_PT; j++)
						xm[j] = est_sample<2>(fm, i + j);
				}
			}
		}
		// the sample before this lane's group: the previous lane's last one; a
		// wave's first lane reads it (the lane before a whole group is whole)
		uint32_t xp = __shfl_up(x[EST_PT - 1u], 1, 64);
		if (need_p && lane == 0u && whole)
			xp = i ? est_sample<W>(f, i - 1u) : 0u;
		if (whole) {
			est_accumulate<EST_PT>(a, x, xp, xm, acc);
		} else if (i < send) {
			// the frame's last, partial group: sample by sample
			for (uint32_t t = i; t < send; t++) {
				const uint32_t x1[1] = {est_sample<W>(f, t)};
				const uint32_t m1[1] = {need_m ? est_sample<2>(fm, t) : 0u};
				est_accumulate<1>(a, x1, need_p && t ? est_sample<W>(f, t - 1u) : 0u, m1, acc);
			}
		}
	}
	// wave shuffle, LDS, one partial per candidate
	for (uint32_t c = 0; c < a.count; c++) {
		uint32_t v = acc[c * 256u];
#pragma unroll
		for (uint32_t o = 32u; o; o >>= 1)
			v += __shfl_xor(v, (int)o, 64);
		if (lane == 0u)
			s_part[c][wave] = v;
	}
	__syncthreads();
	for (uint32_t c = 0; c < a.count; c++) {
		const EstSlot t = a.slot[c];
		if (tid == c) // a slice's sum stays below 2^22
			a.partial[((uint64_t)frame * a.slices + slice) * a.num_cand + t.col()] =
				(uint64_t)(s_part[c][0] + s_part[c][1] + s_part[c][2] + s_part[c][3]) +
				(uint64_t)est_fixed_bits(t) * (send - s0);
	}
}

__global__ __launch_bounds__(256) void est_finish_kernel(const uint64_t *partial, uint32_t frames, uint32_t slices,
							 uint32_t num_cand, uint64_t hdr16, uint64_t *bits,
							 uint32_t *best)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t frame = blockIdx.x * 4u + (threadIdx.x >> 6);
	if (frame >= frames) // whole waves leave
		return;
	uint64_t t = ~0ull;
	if (lane < num_cand) {
		const uint64_t *p = partial + (uint64_t)frame * slices * num_cand + lane;
		t = 0u;
		uint32_t s = 0;
		for (; s + 8u <= slices; s += 8u) { // eight loads in flight: the sum is latency, not bandwidth
			uint64_t v[8];
#pragma unroll
			for (uint32_t u = 0; u < 8u; u++)
				v[u] = p[(uint64_t)(s + u) * num_cand];
#pragma unroll
			for (uint32_t u = 0; u < 8u; u++)
				t += v[u];
		}
		for (; s < slices; s++)
			t += p[(uint64_t)s * num_cand];
		bits[(uint64_t)frame * num_cand + lane] = t;
		t += (hdr16 >> lane) & 1u ? 8u * 16u : 8u * 22u; // the header: bit c of hdr16, 16 bytes, else 22
	}
	if (!best)
		return;
	// argmin of (total, index): lanes past the candidates hold the largest value
	uint32_t idx = lane;
#pragma unroll
	for (uint32_t o = 32u; o; o >>= 1) {
		const uint32_t lo = __shfl_xor((uint32_t)t, (int)o, 64), hi = __shfl_xor((uint32_t)(t >> 32), (int)o, 64);
		const uint32_t oi = __shfl_xor(idx, (int)o, 64);
		const uint64_t ot = ((uint64_t)hi << 32) | lo;
		if (ot < t || (ot == t && oi < idx)) {
			t = ot;
			idx = oi;
		}
	}
	if (lane == 0u)
		best[frame] = idx;
}

} // namespace airsest

using namespace airsest;

static uint64_t g_est_stats[AIRS_EST_STAT_COUNT];

extern "C" uint32_t airs_dev_estimate_stats(uint64_t *out, uint32_t n)
{
	for (uint32_t i = 0; out && i < n && i < AIRS_EST_STAT_COUNT; i++)
		out[i] = __atomic_load_n(&g_est_stats[i], __ATOMIC_RELAXED);
	return AIRS_EST_STAT_COUNT;
}

#define ECHECK(x)                                   \
	do {                                        \
		if ((x) != hipSuccess)              \
			return ERRV(E_GENERIC);     \
	} while (0)

// the sizing launches of the candidates sel[0 .. cnt) over `frames` frames
static uint32_t est_launch_groups(hipStream_t s, const struct airs_estimate *q, const uint32_t *sel, uint32_t cnt,
				  const void *src, uint64_t src_stride, uint32_t sample_bytes, uint32_t as_pre_none,
				  const uint8_t *model, uint32_t frames, uint32_t slices, uint64_t *partial)
{
	for (uint32_t g0 = 0; g0 < cnt; g0 += EST_GROUP) {
		EstArgs a;
		memset(&a, 0, sizeof(a));
		a.src = (const uint8_t *)src;
		a.src_stride = src_stride;
		a.model = model;
		a.model_stride = q->model_stride;
		a.partial = partial;
		a.n = q->n;
		a.slices = slices;
		a.num_cand = q->num_cand;
		a.count = cnt - g0 < EST_GROUP ? cnt - g0 : EST_GROUP;
		for (uint32_t c = 0; c < a.count; c++) {
			const struct airs_est_cand *h = &q->cand[sel[g0 + c]];
			EstSlot *t = &a.slot[c];
			const uint32_t pre = as_pre_none ? PRE_NONE : h->pre;
			t->what = h->kind | pre << 2 | h->k << 4 | ((h->g & (h->g - 1u)) == 0u ? 1u << 8 : 0u) | sel[g0 + c] << 16;
			t->cutoff = h->cutoff;
			t->outlier = h->outlier < 65536u ? h->outlier : 65536u;
			t->rcp = h->rcp;
			a.pre_mask |= 1u << pre;
		}
		if (!((a.pre_mask >> PRE_MODEL) & 1u))
			a.model = nullptr;
		const dim3 grid(slices * frames); // <= 2^31 - 1: the caller's chunks
		if (sample_bytes == 2)
			hipLaunchKernelGGL(est_size_kernel<2>, grid, dim3(256), 0, s, a);
		else
			hipLaunchKernelGGL(est_size_kernel<4>, grid, dim3(256), 0, s, a);
		__atomic_fetch_add(&g_est_stats[AIRS_EST_STAT_SIZE], 1u, __ATOMIC_RELAXED);
	}
	ECHECK(hipGetLastError());
	return 0;
}

extern "C" uint32_t airs_dev_estimate(struct airs_dev_engine *e, const struct airs_estimate *q)
{
	if (!e || !q || !q->src || !q->cand || !q->bits || !q->n || !q->num_frames || !q->num_cand ||
	    q->num_cand > 64u || (q->sample_bytes != 2 && q->sample_bytes != 4))
		return ERRV(E_GENERIC);
	hipStream_t s = (hipStream_t)airs_dev_engine_stream(e);
	uint32_t plain[64], iwt[64], np = 0, ni = 0;
	uint64_t hdr16 = 0u;
	for (uint32_t c = 0; c < q->num_cand; c++) {
		if (q->cand[c].hdr == 16u)
			hdr16 |= 1ull << c;
		if (q->cand[c].pre == 2u && q->cand[c].kind != AIRS_EST_RAW) // CMP_PREPROCESS_IWT (16 bits a sample need no transform)
			iwt[ni++] = c;
		else
			plain[np++] = c;
	}
	const uint32_t slices = (q->n + EST_SLICE - 1u) / EST_SLICE;
	// chunks of frames: the partials within EST_PARTIAL_MAX, the grid within
	// 2^31 - 1 workgroups, the coefficients of IWT candidates within EST_IWT_MAX
	// (AIRS_TEST_ESTIMATE_IWT_FRAMES: frames per chunk instead, tests only); a
	// chunk holds one frame at least
	const uint64_t cstride = ((uint64_t)q->n * 2u + 15u) & ~15ull;
	uint64_t per = EST_PARTIAL_MAX / ((uint64_t)slices * q->num_cand * 8u);
	if (per > 0x7FFFFFFFull / slices)
		per = 0x7FFFFFFFull / slices;
	if (ni) {
		uint64_t ci = EST_IWT_MAX / cstride;
		if (const char *t = getenv("AIRS_TEST_ESTIMATE_IWT_FRAMES"))
			ci = strtoull(t, nullptr, 10);
		if (per > ci)
			per = ci;
	}
	if (per < 1u)
		per = 1u;
	if (per > q->num_frames)
		per = q->num_frames;
	uint64_t *partial = (uint64_t *)airs_dev_scratch(e, AIRS_SLOT_ESTIMATE, (size_t)(per * slices * q->num_cand * 8u));
	uint8_t *coef = ni ? (uint8_t *)airs_dev_scratch(e, AIRS_SLOT_ESTIMATE + 1, (size_t)(per * cstride)) : nullptr;
	if (!partial || (ni && !coef))
		return ERRV(E_GENERIC);
	for (uint32_t f0 = 0; f0 < q->num_frames; f0 += (uint32_t)per) {
		const uint32_t frames = q->num_frames - f0 < per ? q->num_frames - f0 : (uint32_t)per;
		const uint8_t *src = (const uint8_t *)q->src + (uint64_t)f0 * q->src_stride;
		const uint8_t *model = q->model ? (const uint8_t *)q->model + (uint64_t)f0 * q->model_stride : nullptr;
		uint32_t r = 0;
		if (np)
			r = est_launch_groups(s, q, plain, np, src, q->src_stride, q->sample_bytes, 0u, model, frames, slices,
					      partial);
		if (r)
			return r;
		if (ni) {
			// the encoder's transform into scratch, then the coefficients as
			// NONE frames of 16-bit samples
			struct airs_launch L;
			memset(&L, 0, sizeof(L));
			L.src = src;
			L.src_stride = q->src_stride;
			L.sample_bytes = q->sample_bytes;
			L.n = q->n;
			L.num_frames = frames;
			L.frame_mul = 1u;
			L.model = coef;
			L.model_stride = cstride;
			L.model_div = 1u;
			r = airs_dev_iwt(e, &L);
			if (r)
				return r;
			__atomic_fetch_add(&g_est_stats[AIRS_EST_STAT_IWT], 1u, __ATOMIC_RELAXED);
			r = est_launch_groups(s, q, iwt, ni, coef, cstride, 2u, 1u, nullptr, frames, slices, partial);
			if (r)
				return r;
		}
		hipLaunchKernelGGL(est_finish_kernel, dim3((frames + 3u) / 4u), dim3(256), 0, s, partial, frames, slices,
				   q->num_cand, hdr16, q->bits + (uint64_t)f0 * q->num_cand, q->best ? q->best + f0 : nullptr);
		ECHECK(hipGetLastError());
		__atomic_fetch_add(&g_est_stats[AIRS_EST_STAT_FINISH], 1u, __ATOMIC_RELAXED);
	}
	return 0;
}
