/*
 * ck_ragged.hip -- airs_dev_checksum_ragged (airs_dev.h): the XXH32 of frames
 * of different sizes that lie anywhere in device memory, for the ragged pieces
 * of cmp_gpu_compress_image (CMP_GPU_OPT_IMAGE_RAGGED_CHECKSUM, DESIGN.md
 * 3.4.6).  The split is that of ck_pre_kernel / ck_chain_kernel (encode.hip,
 * DESIGN.md 3.2), the geometry is per frame:
 *
 *   ckr_pre_kernel    one workgroup per 256 round quads of one frame (the host
 *                     lists them: airs_ragged_ck_block): a lane forms the four
 *                     stripes of a quad x P2 and writes 64 bytes, accumulator
 *                     q's four rounds at bytes 16 q.  The products of frame j
 *                     start at byte off[j] of the scratch and take its stripes
 *                     rounded up to a quad, so the scratch grows with the
 *                     samples of the piece, not with frames x largest frame.
 *   ckr_chain_kernel  four lanes per frame, sixteen frames per wave, frame
 *                     slot = table index.  A lane reads its accumulator's 16
 *                     bytes of every quad, 128 rounds ahead of the chain, and
 *                     never past its own frame's quads; lanes of a shorter
 *                     frame leave the loop early, lanes of an empty slot read
 *                     and write nothing.  Lane 0 of a frame folds the four
 *                     accumulators and the 0 to 15 byte tail, which it reads
 *                     from the samples.
 *
 * The constants and the four small helpers are restated from encode.hip, which
 * stays as it is: its kernels' code objects are pinned by tests.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "airs_dev.h"

namespace airsck {

#define E_GENERIC 1u
#define E_PARAMS_INVALID 10u
#define ERRV(c) ((uint32_t)0u - (uint32_t)(c))

#define XP1 2654435761u
#define XP2 2246822519u
#define XP3 3266489917u
#define XP4 668265263u
#define XP5 374761393u
#define CK_SEED 419764627u
#define CK_BLOCK_QUADS 256u // round quads per product workgroup (CMP_IMAGE_CK_BLOCK_QUADS)

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

template <int W>
__device__ __forceinline__ uint32_t sample_at(const uint8_t *f, uint32_t i)
{
	return W == 2 ? (uint32_t)reinterpret_cast<const uint16_t *>(f)[i]
		      : reinterpret_cast<const uint32_t *>(f)[i] & 0xFFFFu;
}

// little-endian read of the BE byte image: bytes (hi0, lo0, hi1, lo1)
__device__ __forceinline__ uint32_t be_pair(uint32_t s0, uint32_t s1)
{
	return ((s0 >> 8) & 0xFFu) | ((s0 & 0xFFu) << 8) | (((s1 >> 8) & 0xFFu) << 16) | ((s1 & 0xFFu) << 24);
}

// one XXH32 round with the input's P2 product already formed (encode.hip)
__device__ __forceinline__ uint32_t xxh_round_pre(uint32_t acc, uint32_t yp2)
{
	asm volatile("v_add_u32 %0, %0, %1\n\tv_alignbit_b32 %0, %0, %0, 19\n\tv_mul_lo_u32 %0, %0, %2"
		     : "+v"(acc)
		     : "v"(yp2), "s"(XP1));
	return acc;
}

template <int W>
__global__ __launch_bounds__(256) void ckr_pre_kernel(CkTabs t, const airs_ragged_ck_block *blocks)
{
	const airs_ragged_ck_block b = blocks[blockIdx.x];
	const uint32_t stripes = t.n[b.frame] / 8u;
	const uint32_t r4 = b.qb * CK_BLOCK_QUADS + threadIdx.x; // this lane's round quad
	if ((uint64_t)4u * r4 >= stripes)
		return;
	const uint8_t *f = reinterpret_cast<const uint8_t *>((uintptr_t)t.src[b.frame]);
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
		// a frame base off the 16-byte grid, or the frame's last, partial quad:
		// sample by sample, nothing past stripe `stripes`
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
	uint4 *G = reinterpret_cast<uint4 *>(t.Y + t.off[b.frame]) + (uint64_t)r4 * 4u;
#pragma unroll
	for (uint32_t q = 0; q < 4u; q++)
		G[q] = make_uint4(y[0][q] * XP2, y[1][q] * XP2, y[2][q] * XP2, y[3][q] * XP2);
}

template <int W>
__global__ __launch_bounds__(64) void ckr_chain_kernel(CkTabs t, uint32_t frames, uint32_t *out)
{
	const uint32_t lane = threadIdx.x, q = lane & 3u;
	const uint32_t slot = blockIdx.x * 16u + (lane >> 2);
	const bool valid = slot < frames;
	const uint32_t n = valid ? t.n[slot] : 0u;
	const uint32_t len = 2u * n;
	const uint32_t stripes = n / 8u; // 0: under 16 bytes (and every lane of an empty slot)
	uint32_t acc = q == 0 ? CK_SEED + XP1 + XP2 : q == 1 ? CK_SEED + XP2 : q == 2 ? CK_SEED : CK_SEED - XP1;
	// this lane's chain: 16 bytes (4 rounds) of every 64-byte quad of its frame;
	// dereferenced for quads below ceil(stripes / 4) only
	const uint4 *P = reinterpret_cast<const uint4 *>(t.Y + (valid ? t.off[slot] : 0ull)) + q;
	// batches of 128 rounds (32 x 16 bytes per lane), the next batch loading
	// while this one runs; the last batch reloads itself
	constexpr uint32_t B = 32u;
	const uint32_t nb = stripes / (4u * B);
	uint4 cur[B], nxt[B];
	if (nb) {
#pragma unroll
		for (uint32_t u = 0; u < B; u++)
			cur[u] = P[4u * u];
	}
	for (uint32_t b = 0; b < nb; b++) {
		const uint32_t nbase = (b + 1u < nb ? b + 1u : b) * B;
#pragma unroll
		for (uint32_t u = 0; u < B; u++)
			nxt[u] = P[4u * (nbase + u)];
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
		acc = xxh_round_pre(acc, reinterpret_cast<const uint32_t *>(P + 4u * (r >> 2))[r & 3u]);
	const uint32_t a1 = __shfl_down(acc, 1, 4), a2 = __shfl_down(acc, 2, 4), a3 = __shfl_down(acc, 3, 4);
	if (q != 0 || !valid || !n)
		return;
	const uint8_t *f = reinterpret_cast<const uint8_t *>((uintptr_t)t.src[slot]);
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
	out[slot] = h;
}

// ragged checksum launches and the frames they covered (airs_dev_ragged_ck_stats)
static std::atomic<uint64_t> g_stats[AIRS_RAGGED_CK_STAT_COUNT];

} // namespace airsck

using namespace airsck;

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
	// the device layer's checksum-products slot (airs_dev_checksum's); never an
	// empty request: a slot that was never allocated has no address
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
	if (hipGetLastError() != hipSuccess)
		return ERRV(E_GENERIC);
	g_stats[AIRS_RAGGED_CK_STAT_LAUNCHES].fetch_add(1u, std::memory_order_relaxed);
	g_stats[AIRS_RAGGED_CK_STAT_FRAMES].fetch_add(q->frames, std::memory_order_relaxed);
	return 0;
}
