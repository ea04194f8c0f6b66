/*
 * checksum.hip -- the device checksum (airs_dev.h: airs_dev_checksum,
 * airs_dev_checksum_n, airs_dev_checksum_ragged): XXH32 per frame, seed
 * 419764627, over the samples as big-endian 16-bit words (reference
 * header.c:137-163).  A stripe is 8 samples = 16 bytes; the four accumulators
 * of a frame run in four lanes, lane q consumes bytes 4q..4q+3 of every stripe.
 *
 * Two launches: a product kernel forms every stripe's four
 * inputs x P2 (the multiply taken off the chain) into a scratch buffer with all
 * the parallelism of the frame, one round quad (4 stripes, 64 bytes of
 * products) per lane and pass; a chain kernel then runs only the serial
 * accumulator chains, 16 frames per wave, reading its products 128 rounds
 * ahead, and lane 0 of a frame folds the four accumulators and the 0 to 15
 * byte tail, which it reads from the samples.  That text exists once
 * (ck_quad_products, ck_chain_rounds, ck_finish); the kernels are the two
 * geometries it runs in:
 *
 *   strided  ck_pre_kernel / ck_chain_kernel: frames at src + frame * stride,
 *            chosen by an optional frame list; one size n for all of them, or
 *            (VN, the decoder's verification) frame f has frame_n[f] samples
 *            (0: none, nothing is written for it) and n is the largest of them
 *            and sizes the scratch.  The products are laid out for the chain
 *            wave: per group of 16 frames, for every 4 rounds, 64 chains x 16
 *            bytes (chain = 4 (frame % 16) + accumulator), so one 16-byte load
 *            per lane reads 1 KiB contiguous.  S4 = stripes rounded up to 4.
 *   ragged   ckr_pre_kernel / ckr_chain_kernel: frames of different sizes that
 *            lie anywhere in device memory, for the ragged pieces of
 *            cmp_gpu_compress_image (CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM,
 *            DESIGN.md 3.4.6).  The host lists the product workgroups, one per
 *            256 round quads of one frame (airs_ragged_ck_block).  The products
 *            of frame j start at byte off[j] of the scratch and take its
 *            stripes rounded up to a quad, accumulator q's four rounds at bytes
 *            16 q of a quad, so the scratch grows with the samples of the
 *            piece, not with frames x largest frame.  Frame slot = table index.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "airs_dev.h"
#include "cmp_image_plan.h"
#include "enc_common.h"

namespace airs {

#define XP1 2654435761u
#define XP2 2246822519u
#define XP3 3266489917u
#define XP4 668265263u
#define XP5 374761393u
#define CK_SEED 419764627u
// accumulator q's start value
#define CK_ACC_INIT(q) ((q) == 0 ? CK_SEED + XP1 + XP2 : (q) == 1 ? CK_SEED + XP2 : (q) == 2 ? CK_SEED : CK_SEED - XP1)

struct CkTabs {
	const uint64_t *src; // [frames]: address of the first sample
	const uint32_t *n;   // [frames]: samples
	const uint64_t *off; // [frames]: byte offset of the products in Y
	uint8_t *Y;
};

__device__ __forceinline__ uint32_t rotl32(uint32_t x, uint32_t r)
{
	return (x << r) | (x >> (32u - r));
}

// little-endian read of the BE byte image: bytes (hi0, lo0, hi1, lo1)
__device__ __forceinline__ uint32_t be_pair(uint32_t s0, uint32_t s1)
{
	return ((s0 >> 8) & 0xFFu) | ((s0 & 0xFFu) << 8) | (((s1 >> 8) & 0xFFu) << 16) | ((s1 & 0xFFu) << 24);
}

// one XXH32 round with the input's P2 product already formed: add, rotate,
// multiply as three dependent instructions (the compiler would fuse the add
// into a 64-bit v_mad_u64_u32, whose latency is longer)
__device__ __forceinline__ uint32_t xxh_round_pre(uint32_t acc, uint32_t yp2)
{
	asm volatile("v_add_u32 %0, %0, %1\n\tv_alignbit_b32 %0, %0, %0, 19\n\tv_mul_lo_u32 %0, %0, %2"
		     : "+v"(acc)
		     : "v"(yp2), "s"(XP1));
	return acc;
}

// The products of this lane's round quads of the frame at f.  STRIDE: quads r4,
// r4 + step, ... while 4 r4 < stripes (the strided kernel's grid-stride loop);
// otherwise the one quad r4, of which the caller knows 4 r4 < stripes.  Quad r's
// products go to G0 + r * gstep: accumulator q's four rounds in G[q].  The loop
// is here and not in the kernel because the compiler allocates a body it inlines
// into a loop otherwise than a loop it inlines whole.
template <int W, bool STRIDE>
__device__ __forceinline__ void ck_quad_products(const uint8_t *f, uint32_t stripes, uint32_t r4, uint32_t step,
						 uint4 *G0, uint32_t gstep)
{
	for (; !STRIDE || 4u * r4 < stripes; r4 += step) {
		uint32_t y[4][4]; // [round][accumulator]
		if (4u * r4 + 4u <= stripes && ((uintptr_t)f & 15u) == 0u) {
#pragma unroll
			for (uint32_t k = 0; k < 4u; k++) {
				const uint32_t r = 4u * r4 + k;
				if (W == 2) {
					const uint4 v = reinterpret_cast<const uint4 *>(f)[r];
					y[k][0] = __builtin_amdgcn_perm(v.x, v.x, 0x02030001u);
					y[k][1] = __builtin_amdgcn_perm(v.y, v.y, 0x02030001u);
					y[k][2] = __builtin_amdgcn_perm(v.z, v.z, 0x02030001u);
					y[k][3] = __builtin_amdgcn_perm(v.w, v.w, 0x02030001u);
				} else {
					const uint4 lo = reinterpret_cast<const uint4 *>(f)[2u * r];
					const uint4 hi = reinterpret_cast<const uint4 *>(f)[2u * r + 1u];
					y[k][0] = be_pair(lo.x & 0xFFFFu, lo.y & 0xFFFFu);
					y[k][1] = be_pair(lo.z & 0xFFFFu, lo.w & 0xFFFFu);
					y[k][2] = be_pair(hi.x & 0xFFFFu, hi.y & 0xFFFFu);
					y[k][3] = be_pair(hi.z & 0xFFFFu, hi.w & 0xFFFFu);
				}
			}
		} else {
			// a frame base off the 16-byte grid, or the frame's last, partial
			// quad: sample by sample, nothing past stripe `stripes`
#pragma unroll
			for (uint32_t k = 0; k < 4u; k++) {
				const uint32_t r = 4u * r4 + k;
#pragma unroll
				for (uint32_t q = 0; q < 4u; q++)
					y[k][q] = r < stripes ? be_pair(sample_at<W>(f, 8u * r + 2u * q),
								     sample_at<W>(f, 8u * r + 2u * q + 1u))
							   : 0u;
			}
		}
		uint4 *G = G0 + (uint64_t)r4 * gstep;
#pragma unroll
		for (uint32_t q = 0; q < 4u; q++)
			G[q] = make_uint4(y[0][q] * XP2, y[1][q] * XP2, y[2][q] * XP2, y[3][q] * XP2);
		if (!STRIDE)
			break;
	}
}

// One accumulator's chain over `stripes` rounds.  P is the lane's 16 bytes (4
// rounds) of its frame's first quad, STEP the uint4 distance to those of the
// next quad; quads at and above ceil(stripes / 4) are not dereferenced.
// Batches of 128 rounds (32 x 16 bytes per lane), the next batch loading while
// this one runs; the last batch reloads itself.
template <uint32_t STEP>
__device__ __forceinline__ uint32_t ck_chain_rounds(const uint4 *P, uint32_t stripes, uint32_t acc)
{
	constexpr uint32_t B = 32u;
	const uint32_t nb = stripes / (4u * B);
	uint4 cur[B], nxt[B];
	if (nb) {
#pragma unroll
		for (uint32_t u = 0; u < B; u++)
			cur[u] = P[STEP * u];
	}
	for (uint32_t b = 0; b < nb; b++) {
		const uint32_t nbase = (b + 1u < nb ? b + 1u : b) * B;
#pragma unroll
		for (uint32_t u = 0; u < B; u++)
			nxt[u] = P[STEP * (nbase + u)];
#pragma unroll
		for (uint32_t u = 0; u < B; u++) {
			acc = xxh_round_pre(acc, cur[u].x);
			acc = xxh_round_pre(acc, cur[u].y);
			acc = xxh_round_pre(acc, cur[u].z);
			acc = xxh_round_pre(acc, cur[u].w);
		}
#pragma unroll
		for (uint32_t u = 0; u < B; u++)
			cur[u] = nxt[u];
	}
	for (uint32_t r = nb * 4u * B; r < stripes; r++)
		acc = xxh_round_pre(acc, reinterpret_cast<const uint32_t *>(P + STEP * (r >> 2))[r & 3u]);
	return acc;
}

// The checksum of the n > 0 samples at f from the four accumulators after
// `stripes` = n / 8 rounds: the fold, the length, the tail of 0 to 15 bytes
// and the avalanche.
template <int W>
__device__ __forceinline__ uint32_t ck_finish(const uint8_t *f, uint32_t n, uint32_t stripes, uint32_t acc,
					      uint32_t a1, uint32_t a2, uint32_t a3)
{
	const uint32_t len = 2u * n;
	uint32_t h = stripes ? rotl32(acc, 1) + rotl32(a1, 7) + rotl32(a2, 12) + rotl32(a3, 18) : CK_SEED + XP5;
	h += len;
	uint32_t i = 8u * stripes;
	const uint32_t rem_bytes = len - 16u * stripes;
	uint32_t bb = 0;
	for (; bb + 4u <= rem_bytes; bb += 4u, i += 2u)
		h = rotl32(h + be_pair(sample_at<W>(f, i), sample_at<W>(f, i + 1u)) * XP3, 17) * XP4;
	if (bb < rem_bytes) {
		const uint32_t s0 = sample_at<W>(f, i);
		h = rotl32(h + ((s0 >> 8) & 0xFFu) * XP5, 11) * XP1;
		h = rotl32(h + (s0 & 0xFFu) * XP5, 11) * XP1;
	}
	h ^= h >> 15;
	h *= XP2;
	h ^= h >> 13;
	h *= XP3;
	h ^= h >> 16;
	return h;
}

template <int W, bool VN>
__global__ __launch_bounds__(256) void ck_pre_kernel(const uint8_t *src, uint64_t stride, uint32_t n,
						     uint32_t num_frames, const uint32_t *frame_list, uint32_t S4,
						     uint32_t *Y, const uint32_t *frame_n)
{
	// a workgroup covers 16 frames x 16 round quads, frame fastest: the 64
	// lanes of a wave write 4 KiB of Y contiguous (their four stores fill it)
	const uint32_t lf = blockIdx.x * 16u + (threadIdx.x & 15u);
	if (lf >= num_frames)
		return;
	const uint32_t frame = frame_list ? frame_list[lf] : lf;
	const uint32_t stripes = (VN ? frame_n[frame] : n) / 8u;
	const uint8_t *f = src + (uint64_t)frame * stride;
	// grid-stride: gridDim.y is capped
	ck_quad_products<W, true>(f, stripes, blockIdx.y * 16u + (threadIdx.x >> 4), gridDim.y * 16u,
				  reinterpret_cast<uint4 *>(Y + (uint64_t)(lf >> 4) * 64u * S4) + (lf & 15u) * 4u, 64u);
}

template <int W, bool VN>
__global__ __launch_bounds__(64) void ck_chain_kernel(const uint8_t *src, uint64_t stride, uint32_t n0,
						      uint32_t num_frames, const uint32_t *frame_list, uint32_t S4,
						      const uint32_t *Y, uint32_t *out, const uint32_t *frame_n)
{
	const uint32_t lane = threadIdx.x, q = lane & 3u;
	const uint32_t lf = blockIdx.x * 16u + (lane >> 2);
	const bool valid = lf < num_frames;
	const uint32_t n = !VN ? n0 : valid ? frame_n[frame_list ? frame_list[lf] : lf] : 0u;
	const uint32_t stripes = n / 8u; // 0: under 16 bytes
	// this lane's chain: 16 bytes (4 rounds) every 1 KiB of its group
	const uint4 *P = reinterpret_cast<const uint4 *>(Y + (uint64_t)blockIdx.x * 64u * S4) + lane;
	const uint32_t acc = ck_chain_rounds<64u>(P, stripes, CK_ACC_INIT(q));
	const uint32_t a1 = __shfl_down(acc, 1, 4), a2 = __shfl_down(acc, 2, 4), a3 = __shfl_down(acc, 3, 4);
	if (q != 0 || !valid || !n)
		return;
	const uint32_t frame = frame_list ? frame_list[lf] : lf;
	out[frame] = ck_finish<W>(src + (uint64_t)frame * stride, n, stripes, acc, a1, a2, a3);
}

template <int W>
__global__ __launch_bounds__(256) void ckr_pre_kernel(CkTabs t, const airs_ragged_ck_block *blocks)
{
	const airs_ragged_ck_block b = blocks[blockIdx.x];
	const uint32_t stripes = t.n[b.frame] / 8u;
	const uint32_t r4 = b.qb * CMP_IMAGE_CK_BLOCK_QUADS + threadIdx.x; // this lane's round quad
	if ((uint64_t)4u * r4 >= stripes)
		return;
	const uint8_t *f = reinterpret_cast<const uint8_t *>((uintptr_t)t.src[b.frame]);
	ck_quad_products<W, false>(f, stripes, r4, 0u, reinterpret_cast<uint4 *>(t.Y + t.off[b.frame]), 4u);
}

template <int W>
__global__ __launch_bounds__(64) void ckr_chain_kernel(CkTabs t, uint32_t frames, uint32_t *out)
{
	const uint32_t lane = threadIdx.x, q = lane & 3u;
	const uint32_t slot = blockIdx.x * 16u + (lane >> 2);
	const bool valid = slot < frames;
	const uint32_t n = valid ? t.n[slot] : 0u;
	const uint32_t stripes = n / 8u; // 0: under 16 bytes (and every lane of an empty slot)
	// this lane's chain: 16 bytes (4 rounds) of every 64-byte quad of its frame
	const uint4 *P = reinterpret_cast<const uint4 *>(t.Y + (valid ? t.off[slot] : 0ull)) + q;
	const uint32_t acc = ck_chain_rounds<4u>(P, stripes, CK_ACC_INIT(q));
	const uint32_t a1 = __shfl_down(acc, 1, 4), a2 = __shfl_down(acc, 2, 4), a3 = __shfl_down(acc, 3, 4);
	if (q != 0 || !valid || !n)
		return;
	const uint8_t *f = reinterpret_cast<const uint8_t *>((uintptr_t)t.src[slot]);
	out[slot] = ck_finish<W>(f, n, stripes, acc, a1, a2, a3);
}

// ragged checksum launches and the frames they covered (airs_dev_ragged_ck_stats)
static std::atomic<uint64_t> g_stats[AIRS_RAGGED_CK_STAT_COUNT];

// after a launch pair: 0, or the launch error with its text (airs_dev_last_error)
static uint32_t ck_launched(void)
{
	const hipError_t he = hipGetLastError();
	return he == hipSuccess ? 0u : hip_fail(he, "hipGetLastError()");
}

template <bool VN>
static uint32_t checksum_launch(struct airs_dev_engine *e, const void *src, uint64_t src_stride,
				uint32_t sample_bytes, uint32_t n, uint32_t num_frames, const uint32_t *frame_list,
				uint32_t *out, const uint32_t *frame_n)
{
	if (!e || !n || !num_frames)
		return ERRV(E_GENERIC);
	dim3 grid((num_frames + 15) / 16);
	const uint32_t stripes = n / 8u;
	const uint32_t S4 = (stripes + 3u) & ~3u;
	// whole groups of 16 frames x 4 chains
	// (at least one granule: frames under 8 samples have no stripes, and an
	// empty request would return a slot that was never allocated)
	uint32_t *Y = (uint32_t *)airs_dev_scratch(e, AIRS_NSLOT - 4, (size_t)grid.x * 64u * S4 * 4u + 16u);
	if (!Y)
		return ERRV(E_GENERIC);
	hipStream_t s = (hipStream_t)airs_dev_engine_stream(e);
	if (stripes) {
		const dim3 pg(grid.x, min((S4 / 4u + 15u) / 16u, 65535u));
		if (sample_bytes == 2)
			hipLaunchKernelGGL((ck_pre_kernel<2, VN>), pg, dim3(256), 0, s, (const uint8_t *)src, src_stride,
					   n, num_frames, frame_list, S4, Y, frame_n);
		else
			hipLaunchKernelGGL((ck_pre_kernel<4, VN>), pg, dim3(256), 0, s, (const uint8_t *)src, src_stride,
					   n, num_frames, frame_list, S4, Y, frame_n);
	}
	if (sample_bytes == 2)
		hipLaunchKernelGGL((ck_chain_kernel<2, VN>), grid, dim3(64), 0, s, (const uint8_t *)src, src_stride, n,
				   num_frames, frame_list, S4, (const uint32_t *)Y, out, frame_n);
	else
		hipLaunchKernelGGL((ck_chain_kernel<4, VN>), grid, dim3(64), 0, s, (const uint8_t *)src, src_stride, n,
				   num_frames, frame_list, S4, (const uint32_t *)Y, out, frame_n);
	return ck_launched();
}

} // namespace airs

using namespace airs;

extern "C" uint32_t airs_dev_checksum(struct airs_dev_engine *e, const void *src, uint64_t src_stride,
				      uint32_t sample_bytes, uint32_t n, uint32_t num_frames,
				      const uint32_t *frame_list, uint32_t *out)
{
	return checksum_launch<false>(e, src, src_stride, sample_bytes, n, num_frames, frame_list, out, nullptr);
}

extern "C" uint32_t airs_dev_checksum_n(struct airs_dev_engine *e, const void *src, uint64_t src_stride,
					uint32_t sample_bytes, uint32_t n_max, const uint32_t *frame_n,
					uint32_t num_frames, uint32_t *out)
{
	if (!frame_n)
		return ERRV(E_GENERIC);
	return checksum_launch<true>(e, src, src_stride, sample_bytes, n_max, num_frames, nullptr, out, frame_n);
}

extern "C" uint32_t airs_dev_ragged_ck_stats(uint64_t *out, uint32_t n)
{
	for (uint32_t i = 0; out && i < n && i < AIRS_RAGGED_CK_STAT_COUNT; i++)
		out[i] = g_stats[i].load(std::memory_order_relaxed);
	return AIRS_RAGGED_CK_STAT_COUNT;
}

extern "C" uint32_t airs_dev_checksum_ragged(struct airs_dev_engine *e, const struct airs_ragged_ck *q)
{
	if (!e || !q || !q->frames || !q->src || !q->n || !q->off || !q->out || (q->num_blocks && !q->blocks) ||
	    q->num_blocks > 0x7FFFFFFFu || (q->bytes & 15u))
		return ERRV(E_GENERIC);
	if (q->sample_bytes != 2 && q->sample_bytes != 4)
		return ERRV(E_PARAMS_INVALID);
	// the strided entry points' products slot; never an empty request: a slot
	// that was never allocated has no address
	uint8_t *Y = (uint8_t *)airs_dev_scratch(e, AIRS_NSLOT - 4, (size_t)q->bytes + 16u);
	if (!Y)
		return ERRV(E_GENERIC);
	hipStream_t s = (hipStream_t)airs_dev_engine_stream(e);
	const CkTabs t = {q->src, q->n, q->off, Y};
	const dim3 grid((q->frames + 15u) / 16u);
	if (q->sample_bytes == 2) {
		if (q->num_blocks)
			hipLaunchKernelGGL(ckr_pre_kernel<2>, dim3(q->num_blocks), dim3(256), 0, s, t, q->blocks);
		hipLaunchKernelGGL(ckr_chain_kernel<2>, grid, dim3(64), 0, s, t, q->frames, q->out);
	} else {
		if (q->num_blocks)
			hipLaunchKernelGGL(ckr_pre_kernel<4>, dim3(q->num_blocks), dim3(256), 0, s, t, q->blocks);
		hipLaunchKernelGGL(ckr_chain_kernel<4>, grid, dim3(64), 0, s, t, q->frames, q->out);
	}
	if (const uint32_t r = ck_launched())
		return r;
	g_stats[AIRS_RAGGED_CK_STAT_LAUNCHES].fetch_add(1u, std::memory_order_relaxed);
	g_stats[AIRS_RAGGED_CK_STAT_FRAMES].fetch_add(q->frames, std::memory_order_relaxed);
	return 0;
}
