/*
 * encode_image.hip -- airs_dev_encode_image (airs_dev.h): the device work of
 * cmp_gpu_compress_image (include/cmp_gpu.h) around the batch encoder, per
 * run of equal frames.
 *
 * The batch encoder reads frames at one stride, native-endian and aligned to
 * the sample size, and writes frame rows of one stride.  Three kernels stand
 * around it:
 *
 *   encimage_ingest_kernel  frame j's samples, at any of the 16 byte phases of
 *                         the sample image, into the 16-byte aligned row j:
 *                         aligned 16-byte loads, a byte funnel
 *                         (v_alignbyte_b32), with big-endian sources one
 *                         v_perm_b32 per two samples, aligned 16-byte stores;
 *                         the row is zero from the frame's end to the next
 *                         multiple of 16.  The shape of the decoder's
 *                         img_unpack_kernel plus the swap.
 *   encimage_scan_kernel    one workgroup: the 64-bit, byte-granular offsets of
 *                         the run's frames from their sizes, continued from
 *                         the offset the run before left; a sticky device word
 *                         turns the first frame that passes the capacity and
 *                         every frame after it into CMP_ERR_DST_TOO_SMALL.
 *   encimage_emit_kernel    frame row j to out + out_offsets[j] at any phase: the
 *                         destination's 16-byte lines are stored whole from the
 *                         funnelled row; heads and tails (15 bytes each at
 *                         most) share their lines with the neighbours and are
 *                         stored byte by byte, never read.
 *
 * Both copies run one workgroup per (frame, 16 KiB tile) and use no LDS.  The
 * sizes are known on the device only, so the emit grid covers the row's
 * capacity and the workgroups past the frame's end return at once.
 *
 * A ragged piece (frames of unequal sizes) gives both copies
 * per-frame tables instead of one stride: the ingest a row offset and a length
 * per frame (length 0: the frame is read where it lies, its workgroups return
 * at once), the emit a frame-row offset per frame.  Their grids then cover the
 * largest frame of the piece.  With null tables the kernels behave as above.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "airs_dev.h"
#include "img_copy.h"

namespace airsimg {

#define E_GENERIC 1u
#define E_DST_TOO_SMALL 30u
#define E_MAX_CODE 128u // values above ERRV(E_MAX_CODE) are error values (cmp_errors.h)
#define ERRV(c) ((uint32_t)0u - (uint32_t)(c))
#define ENCIMG_SLICE (1u << 20) // frames per launch of the copies (gridDim.x * 256 stays below 2^32)

struct EncImgArgs {
	const uint8_t *src;     // the sample image
	const uint64_t *off;    // [frames of the launch]: byte offset in src
	uint8_t *rows;          // sample rows, row j at rows + j * row_bytes (16-byte aligned)
	uint32_t row_bytes;
	uint32_t frame_bytes;
	uint32_t swap;
	const uint8_t *frows;   // frame rows, row j at frows + j * frow_bytes (8-byte aligned)
	uint32_t frow_bytes;
	const uint32_t *sizes;  // [frames of the launch]
	const uint64_t *dof;    // [frames of the launch]: byte offset in out
	uint8_t *out;
	// a ragged piece (optional): per-frame row offsets and lengths instead of
	// row_bytes / frame_bytes, per-frame frame-row offsets instead of frow_bytes
	const uint64_t *row_off;
	const uint32_t *row_len;
	const uint64_t *frow_off;
};

// Grid: frames of the launch x 16 KiB tiles of a row.
__global__ __launch_bounds__(IMG_WG) void encimage_ingest_kernel(EncImgArgs a)
{
	const uint32_t f = blockIdx.x;
	const uint32_t len = a.row_len ? a.row_len[f] : a.frame_bytes; // (0: a frame read where it lies)
	const uint32_t fill = (len + 15u) & ~15u;
	const uint32_t t0 = blockIdx.y * IMG_TILE + threadIdx.x * 16u;
	if (blockIdx.y * IMG_TILE >= fill)
		return;
	const uint8_t *s = a.src + a.off[f], *end = s + len;
	uint8_t *row = a.rows + (a.row_off ? a.row_off[f] : (uint64_t)f * a.row_bytes);
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
		if (t < fill) {
			if (a.swap)
				v[i] = make_uint4(img_swap16x2(v[i].x), img_swap16x2(v[i].y), img_swap16x2(v[i].z),
						  img_swap16x2(v[i].w));
			*reinterpret_cast<uint4 *>(row + t) = v[i];
		}
	}
}

// One workgroup.  P(j) = B + the sizes of the frames up to j that are no error
// values never decreases, so "the first frame that does not fit and all after
// it" are the frames with P(j) > cap, and the offset they all share is the
// largest P that fitted.
__global__ __launch_bounds__(IMG_WG) void encimage_scan_kernel(uint32_t *sizes, uint64_t *off, uint32_t *sticky,
							     uint32_t count, uint64_t cap, uint32_t first_run,
							     uint32_t force)
{
	__shared__ uint64_t sh[IMG_WG];
	const uint32_t tid = threadIdx.x;
	uint64_t base = first_run ? 0u : off[0];
	const uint32_t stuck = first_run ? 0u : *sticky;
	uint64_t fitted = base;
	if (first_run && tid == 0u)
		off[0] = 0u;
	for (uint32_t t = 0; t < count; t += IMG_WG) {
		const uint32_t j = t + tid;
		const bool in = j < count;
		const uint32_t s = in ? (force ? force : sizes[j]) : 0u;
		sh[tid] = s > ERRV(E_MAX_CODE) ? 0u : s;
		__syncthreads();
		for (uint32_t d = 1; d < IMG_WG; d <<= 1) {
			const uint64_t x = tid >= d ? sh[tid - d] : 0u;
			__syncthreads();
			sh[tid] += x;
			__syncthreads();
		}
		const uint64_t p = base + sh[tid];
		const bool fit = !stuck && p <= cap;
		const uint32_t fits = (uint32_t)__syncthreads_count(fit);
		if (fits)
			fitted = base + sh[fits - 1u];
		if (in) {
			off[j + 1u] = fit ? p : fitted;
			if (!fit)
				sizes[j] = ERRV(E_DST_TOO_SMALL);
			else if (force)
				sizes[j] = force;
		}
		base += sh[IMG_WG - 1u];
		__syncthreads();
	}
	if (tid == 0u)
		*sticky = (stuck || base > cap) ? 1u : 0u;
}

// Grid: frames of the launch x 16 KiB tiles of a frame row.  The frame's bytes
// at d = out + out_offsets[j]: a head up to the first 16-byte line of out, whole
// lines, a tail; the first workgroup of a frame writes head and tail, one byte
// per lane.
__global__ __launch_bounds__(IMG_WG) void encimage_emit_kernel(EncImgArgs a)
{
	const uint32_t f = blockIdx.x;
	const uint32_t bytes = a.sizes[f];
	if (bytes > ERRV(E_MAX_CODE))
		return;
	const uint8_t *row = a.frows + (a.frow_off ? a.frow_off[f] : (uint64_t)f * a.frow_bytes);
	uint8_t *d = a.out + a.dof[f];
	const uint32_t head = min((uint32_t)((0u - (uintptr_t)d) & 15u), bytes);
	const uint32_t body = (bytes - head) & ~15u;
	if (blockIdx.y == 0u && threadIdx.x < 32u) {
		const bool tail = threadIdx.x >= 16u;
		const uint32_t pos = (tail ? head + body : 0u) + (threadIdx.x & 15u);
		if (pos < (tail ? bytes : head))
			d[pos] = row[pos];
	}
	if (blockIdx.y * IMG_TILE >= body)
		return;
	const uint32_t t0 = blockIdx.y * IMG_TILE + threadIdx.x * 16u;
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
		if (t < body)
			*reinterpret_cast<uint4 *>(d + head + t) = v[i];
	}
}

} // namespace airsimg

using namespace airsimg;

// frames through each stage, counted where the kernels are launched (airs_dev_encode_image_stats)
static uint64_t g_encimg_stats[AIRS_ENCIMG_STAT_COUNT];

extern "C" uint32_t airs_dev_encode_image_stats(uint64_t *out, uint32_t n)
{
	for (uint32_t i = 0; i < n && i < AIRS_ENCIMG_STAT_COUNT; i++)
		out[i] = __atomic_load_n(&g_encimg_stats[i], __ATOMIC_RELAXED);
	return AIRS_ENCIMG_STAT_COUNT;
}

extern "C" uint32_t airs_dev_encode_image(struct airs_dev_engine *e, const struct airs_encode_image *q)
{
	if (!e || !q || !q->count)
		return ERRV(E_GENERIC);
	hipStream_t s = (hipStream_t)airs_dev_engine_stream(e);
	EncImgArgs a;
	memset(&a, 0, sizeof(a));
	if (q->stage == AIRS_ENCIMG_INGEST) {
		if (!q->src || !q->offsets || !q->rows || !q->frame_bytes || ((uintptr_t)q->rows & 15u) ||
		    (!q->row_len && ((q->row_bytes & 15u) || q->row_bytes < q->frame_bytes)) || !q->row_len != !q->row_off)
			return ERRV(E_GENERIC);
		a.src = (const uint8_t *)q->src;
		a.row_bytes = q->row_bytes;
		a.frame_bytes = q->frame_bytes;
		a.swap = q->swap;
		const uint32_t tiles = (uint32_t)(((uint64_t)q->frame_bytes + IMG_TILE - 1u) / IMG_TILE);
		if (tiles > 65535u)
			return ERRV(E_GENERIC);
		for (uint32_t j = 0; j < q->count; j += ENCIMG_SLICE) {
			const uint32_t cnt = q->count - j < ENCIMG_SLICE ? q->count - j : ENCIMG_SLICE;
			a.off = q->offsets + j;
			a.rows = (uint8_t *)q->rows + (q->row_len ? 0u : (uint64_t)j * q->row_bytes);
			a.row_off = q->row_off ? q->row_off + j : nullptr;
			a.row_len = q->row_len ? q->row_len + j : nullptr;
			hipLaunchKernelGGL(encimage_ingest_kernel, dim3(cnt, tiles), dim3(IMG_WG), 0, s, a);
		}
		__atomic_fetch_add(&g_encimg_stats[AIRS_ENCIMG_STAT_INGEST], q->row_len ? q->staged : q->count,
				   __ATOMIC_RELAXED);
	} else if (q->stage == AIRS_ENCIMG_EMIT) {
		if (!q->sizes || !q->out_offsets || !q->sticky || !q->out || (!q->force && !q->frows) ||
		    (!q->frow_off && ((q->frow_bytes & 7u) || q->frow_bytes < q->frow_cap)))
			return ERRV(E_GENERIC);
		hipLaunchKernelGGL(encimage_scan_kernel, dim3(1), dim3(IMG_WG), 0, s, q->sizes, q->out_offsets, q->sticky,
				   q->count, q->out_capacity, q->first_run, q->force);
		__atomic_fetch_add(&g_encimg_stats[q->force ? AIRS_ENCIMG_STAT_REFUSED : AIRS_ENCIMG_STAT_EMIT], q->count,
				   __ATOMIC_RELAXED);
		if (!q->force) {
			a.frow_bytes = q->frow_bytes;
			a.out = (uint8_t *)q->out;
			const uint32_t tiles = (uint32_t)(((uint64_t)q->frow_cap + IMG_TILE - 1u) / IMG_TILE);
			if (tiles > 65535u)
				return ERRV(E_GENERIC);
			for (uint32_t j = 0; j < q->count; j += ENCIMG_SLICE) {
				const uint32_t cnt = q->count - j < ENCIMG_SLICE ? q->count - j : ENCIMG_SLICE;
				a.frows = (const uint8_t *)q->frows + (q->frow_off ? 0u : (uint64_t)j * q->frow_bytes);
				a.frow_off = q->frow_off ? q->frow_off + j : nullptr;
				a.sizes = q->sizes + j;
				a.dof = q->out_offsets + j;
				hipLaunchKernelGGL(encimage_emit_kernel, dim3(cnt, tiles ? tiles : 1u), dim3(IMG_WG), 0, s,
						   a);
			}
		}
	} else {
		return ERRV(E_GENERIC);
	}
	if (hipGetLastError() != hipSuccess)
		return ERRV(E_GENERIC);
	return 0;
}
