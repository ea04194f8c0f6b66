/*
 * decode_image.hip -- airs_dev_decode_image (airs_dev.h): frames at arbitrary
 * byte offsets of one device buffer, decoded as one context into samples
 * packed back to back (cmp_gpu_decompress_image, include/cmp_gpu.h).
 *
 * The frame decoder (decode.hip) wants frames in 8-byte aligned rows of one
 * width and writes rows of one width.  Three kernels stand around it:
 *
 *   img_hdr_kernel     one lane per frame: the compressed and the original
 *                      size from the header at src + offsets[f], or "unusable";
 *                      one read-back gives the host the output layout and the
 *                      chunks (cmp_image_plan.c).
 *   img_unpack_kernel  frame f's bytes, at any of the 16 byte phases, into row
 *                      f of the chunk's staging: aligned 16-byte loads, a byte
 *                      funnel (v_alignbyte_b32), aligned 16-byte stores; the row
 *                      is zero from the frame's end to the next multiple of 16
 *                      (the decoder reads whole words).  An unusable slice
 *                      becomes a zero header, which the decoder answers with
 *                      CMP_ERR_INT_HDR.
 *   img_emit_kernel    decoded row f to dst + dst_offsets[f] (2-byte aligned):
 *                      the destination's 16-byte lines are stored whole from
 *                      the funnelled row, heads and tails sample by sample;
 *                      the big-endian form swaps with one v_perm_b32 per two
 *                      samples.
 *
 * Both copies run one workgroup per (frame, 16 KiB tile), so a large frame
 * spreads over the chip, and neither uses LDS.  Between them each chunk is one
 * airs_dev_decode_seq call with one context; the model passes from chunk to
 * chunk in device memory.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "airs_dev.h"
#include "cmp_image_plan.h"
#include "img_copy.h"

namespace airsimg {

#define E_GENERIC 1u
#define E_DST_TOO_SMALL 30u
#define ERRV(c) ((uint32_t)0u - (uint32_t)(c))

struct ImgArgs {
	const uint8_t *src;   // the image
	const uint64_t *off;  // [frames of the chunk]: byte offset in src
	const uint2 *hdr;     // [frames of the chunk]: compressed size (0: unusable), original size
	const uint64_t *dof;  // [frames of the chunk]: byte offset in dst
	uint8_t *rows;        // staged frames, row f at rows + f * row_bytes (16-byte aligned)
	uint32_t row_bytes;
	const uint8_t *drows; // decoded samples, row f at drows + f * drow_bytes (16-byte aligned)
	uint32_t drow_bytes;
	uint8_t *dst;
	uint32_t swap;
};

// header bytes 2..7 of every frame -> (compressed size, original size), or
// (0, 0) for a slice the call cannot use (cmp_gpu.h)
__global__ void img_hdr_kernel(const uint8_t *src, uint64_t src_size, const uint64_t *off, uint2 *hdr, uint32_t n)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f >= n)
		return;
	const uint64_t o = off[f];
	uint2 r = make_uint2(0u, 0u);
	if (src_size >= 16u && o <= src_size - 16u) {
		const uint8_t *b = src + o;
		const uint32_t csize = ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 8) | b[4];
		const uint32_t osize = ((uint32_t)b[5] << 16) | ((uint32_t)b[6] << 8) | b[7];
		if (csize >= 16u && csize <= src_size - o && !(osize & 1u))
			r = make_uint2(csize, osize);
	}
	hdr[f] = r;
}

// Grid: 16 KiB tiles of a row x frames of the chunk.
__global__ __launch_bounds__(IMG_WG) void img_unpack_kernel(ImgArgs a)
{
	const uint32_t f = blockIdx.y;
	const uint32_t len = a.hdr[f].x; // 0: an unusable slice, its offset is never used
	// the header the decoder looks at (22 bytes at most) is always written
	const uint32_t fill = max((len + 15u) & ~15u, (uint32_t)CMP_IMAGE_ROW_MIN);
	const uint32_t t0 = blockIdx.x * IMG_TILE + threadIdx.x * 16u;
	if (blockIdx.x * IMG_TILE >= fill)
		return;
	const uint8_t *s = a.src + a.off[f], *end = s + len;
	uint8_t *row = a.rows + (uint64_t)f * a.row_bytes;
	uint4 v[IMG_LINES];
#pragma unroll
	for (uint32_t i = 0; i < IMG_LINES; i++) {
		const uint32_t t = t0 + i * IMG_WG * 16u;
		v[i] = make_uint4(0u, 0u, 0u, 0u);
		if (t < len) {
			v[i] = img_fetch16(s + t, end);
			if (len - t < 16u)
				v[i] = img_keep(v[i], len - t);
		}
	}
#pragma unroll
	for (uint32_t i = 0; i < IMG_LINES; i++) {
		const uint32_t t = t0 + i * IMG_WG * 16u;
		if (t < fill)
			*reinterpret_cast<uint4 *>(row + t) = v[i];
	}
}

// Grid: 16 KiB tiles of a decoded row x frames of the chunk.  The frame's
// bytes at d = dst + dst_offsets[f]: a head up to the first 16-byte line of
// dst, whole lines, a tail; the first workgroup of a frame writes head and
// tail sample by sample (7 samples each at most).
__global__ __launch_bounds__(IMG_WG) void img_emit_kernel(ImgArgs a)
{
	const uint32_t f = blockIdx.y;
	const uint2 hd = a.hdr[f];
	const uint32_t bytes = hd.x ? hd.y : 0u;
	if (!bytes)
		return;
	const uint8_t *row = a.drows + (uint64_t)f * a.drow_bytes;
	uint8_t *d = a.dst + a.dof[f];
	const uint32_t head = min((uint32_t)((0u - (uintptr_t)d) & 15u), bytes);
	const uint32_t body = (bytes - head) & ~15u;
	if (blockIdx.x == 0u && threadIdx.x < 16u) {
		const bool tail = threadIdx.x >= 8u;
		const uint32_t pos = (tail ? head + body : 0u) + 2u * (threadIdx.x & 7u);
		if (pos < (tail ? bytes : head)) {
			uint32_t v = *reinterpret_cast<const uint16_t *>(row + pos);
			if (a.swap)
				v = (v >> 8) | (v << 8);
			*reinterpret_cast<uint16_t *>(d + pos) = (uint16_t)v;
		}
	}
	if (blockIdx.x * IMG_TILE >= body)
		return;
	const uint32_t t0 = blockIdx.x * IMG_TILE + threadIdx.x * 16u;
	const uint8_t *s = row + head, *end = row + bytes;
	uint4 v[IMG_LINES];
#pragma unroll
	for (uint32_t i = 0; i < IMG_LINES; i++) {
		const uint32_t t = t0 + i * IMG_WG * 16u;
		v[i] = make_uint4(0u, 0u, 0u, 0u);
		if (t < body)
			v[i] = img_fetch16(s + t, end);
	}
#pragma unroll
	for (uint32_t i = 0; i < IMG_LINES; i++) {
		const uint32_t t = t0 + i * IMG_WG * 16u;
		if (t < body) {
			if (a.swap)
				v[i] = make_uint4(img_swap16x2(v[i].x), img_swap16x2(v[i].y), img_swap16x2(v[i].z),
						  img_swap16x2(v[i].w));
			*reinterpret_cast<uint4 *>(d + head + t) = v[i];
		}
	}
}

} // namespace airsimg

using namespace airsimg;

#define ICHECK(x)                               \
	do {                                    \
		if ((x) != hipSuccess)          \
			return ERRV(E_GENERIC); \
	} while (0)

extern "C" uint32_t airs_dev_decode_image(struct airs_dev_engine *e, const struct airs_decode_image *q)
{
	if (!e || !q || !q->src || !q->src_size || !q->offsets || !q->num_frames || !q->dst || ((uintptr_t)q->dst & 1u) ||
	    !q->dst_offsets || !q->status || (q->model && (!q->model_n || !q->model_samples)) ||
	    (q->model_in && !q->model))
		return ERRV(E_GENERIC);
	hipStream_t s = (hipStream_t)airs_dev_engine_stream(e);
	const size_t N = q->num_frames;
	// host and device tables, 8 bytes per entry: offsets [N], headers [N], dst offsets [N + 1]
	uint64_t *h_off = (uint64_t *)airs_dev_host_scratch(e, (3u * N + 1u) * 8u);
	uint64_t *d_off = (uint64_t *)airs_dev_scratch(e, AIRS_SLOT_IMAGE, (3u * N + 1u) * 8u);
	if (!h_off || !d_off)
		return ERRV(E_GENERIC);
	uint32_t *h_hdr = (uint32_t *)(h_off + N);
	uint64_t *h_dof = h_off + 2u * N;
	uint2 *d_hdr = (uint2 *)(d_off + N);
	uint64_t *d_dof = d_off + 2u * N;
	memcpy(h_off, q->offsets, N * 8u);
	ICHECK(hipMemcpyAsync(d_off, h_off, N * 8u, hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(img_hdr_kernel, dim3((uint32_t)((N + 255u) / 256u)), dim3(256), 0, s, (const uint8_t *)q->src,
			   q->src_size, (const uint64_t *)d_off, d_hdr, q->num_frames);
	ICHECK(hipMemcpyAsync(h_hdr, d_hdr, N * 8u, hipMemcpyDeviceToHost, s));
	ICHECK(hipStreamSynchronize(s));
	// the output layout, and the planner's view of the frames: compressed size, samples
	uint64_t total = 0;
	uint32_t nmax = 1;
	for (size_t f = 0; f < N; f++) {
		const uint32_t n = h_hdr[2u * f] ? h_hdr[2u * f + 1u] / 2u : 0u;
		h_dof[f] = total;
		total += 2ull * n;
		h_hdr[2u * f + 1u] = n;
		nmax = n > nmax ? n : nmax;
	}
	h_dof[N] = total;
	memcpy(q->dst_offsets, h_dof, (N + 1u) * 8u);
	if (total > q->dst_capacity)
		return ERRV(E_DST_TOO_SMALL);
	if (q->model && nmax > q->model_samples)
		return ERRV(E_GENERIC);
	ICHECK(hipMemcpyAsync(d_dof, h_dof, (N + 1u) * 8u, hipMemcpyHostToDevice, s));

	// the staging of the largest chunk, allocated once: growing it between
	// chunks would wait for the stream
	struct cmp_image_chunk c;
	size_t stage_bytes = 0;
	uint64_t chunks = 0;
	for (uint64_t first = 0; first < N; first += c.count, chunks++) {
		cmp_image_plan_next(h_hdr, N, q->chunk_bytes, first, &c);
		const size_t need = (size_t)c.count * ((size_t)c.src_cap + c.dst_stride);
		stage_bytes = need > stage_bytes ? need : stage_bytes;
	}
	uint8_t *stage = (uint8_t *)airs_dev_scratch(e, AIRS_SLOT_IMAGE + 1, stage_bytes);
	if (!stage)
		return ERRV(E_GENERIC);
	uint16_t *model = q->model;
	uint32_t *model_n = q->model_n;
	if (chunks > 1u && !model) {
		// no model buffer of the caller's to carry the context from chunk to chunk in
		const size_t mb = ((size_t)2u * nmax + 15u) & ~(size_t)15u;
		uint8_t *m = (uint8_t *)airs_dev_scratch(e, AIRS_SLOT_IMAGE + 2, mb + 16u);
		if (!m)
			return ERRV(E_GENERIC);
		model = (uint16_t *)m;
		model_n = (uint32_t *)(m + mb);
	}
	for (uint64_t first = 0, chunk = 0; first < N; chunk++) {
		cmp_image_plan_next(h_hdr, N, q->chunk_bytes, first, &c);
		ImgArgs a;
		memset(&a, 0, sizeof(a));
		a.src = (const uint8_t *)q->src;
		a.off = d_off + first;
		a.hdr = d_hdr + first;
		a.dof = d_dof + first;
		a.rows = stage;
		a.row_bytes = c.src_cap;
		a.drows = stage + (size_t)c.count * c.src_cap;
		a.drow_bytes = c.dst_stride;
		a.dst = (uint8_t *)q->dst;
		a.swap = q->big_endian;
		hipLaunchKernelGGL(img_unpack_kernel, dim3((c.src_cap + IMG_TILE - 1u) / IMG_TILE, c.count), dim3(IMG_WG), 0,
				   s, a);
		struct airs_decode_seq d;
		memset(&d, 0, sizeof(d));
		d.src = a.rows;
		d.src_stride = c.src_cap;
		d.src_cap = c.src_cap;
		d.num_ctx = 1;
		d.fpc = c.count;
		d.dst = (uint16_t *)a.drows;
		d.dst_stride = c.dst_stride;
		d.dst_samples = c.dst_samples;
		d.status = q->status + first;
		d.model = model;
		d.model_stride = c.dst_stride;
		d.model_n = model_n;
		d.checksum_ok = q->checksum_ok ? q->checksum_ok + first : nullptr;
		d.is_unsigned = q->is_unsigned;
		d.model_in = chunk ? 1u : q->model_in;
		const uint32_t r = airs_dev_decode_seq(e, &d);
		if (r)
			return r;
		hipLaunchKernelGGL(img_emit_kernel, dim3((c.dst_stride + IMG_TILE - 1u) / IMG_TILE, c.count), dim3(IMG_WG), 0,
				   s, a);
		first += c.count;
	}
	ICHECK(hipGetLastError());
	return 0;
}
