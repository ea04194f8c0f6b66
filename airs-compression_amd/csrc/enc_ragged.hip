// enc_ragged.hip -- the ragged encode kernel (cmp_gpu_compress_image with
// CMP_GPU_OPT_IMAGE_RAGGED): frames of different sizes in one
// launch, compiled in its own translation unit.
//
// ragged_kernel does encode_kernel's work (enc_kernel.h) for launches without
// a model, IWT, fused Rice selection or payload-only stream, with its geometry
// per frame instead of per launch.  A block reads one 32-byte descriptor
// (airs_ragged_desc) with a single scalar load before its sample loads: the
// frame's sample address and sample count, the block's segment of the frame,
// the frame's index in the piece and its first granule slot.  Destination
// offset, capacity, identifier and header sequence number come from per-frame
// arrays (RaggedTabs) while the samples are in flight.  Everything after that
// front is encode_kernel's body in its not-FULL, MODEL == 0 form: phase 1, the
// packer, the decoupled look-back of enc_common.h with its bounded spins and
// the fault word, the header, the stores clipped to the frame's capacity.
//
// The host (cmp_image_ragged_blocks, cmp_image_plan.c) orders the blocks by
// segment index, then frame: block (frame, s) is dispatched after (frame,
// s - 1), so a look-back only ever waits on a block dispatched earlier -- the
// condition encode_kernel states for its own order.  There is no other wait.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "enc_kernel.h"

namespace airs {

static_assert(sizeof(airs_ragged_desc) == 32, "one s_load_dwordx8");

template <int W, int PRE, int ENC, bool RICE>
__global__ __launch_bounds__(EWG) void ragged_kernel(KArgs a, RaggedTabs t)
{
	constexpr uint32_t CH = seg_chunks(W, 0);
	constexpr uint32_t SEGN = CH * AIRS_SEG;
	constexpr uint32_t NPIECE = ENC == ENC_MULTI ? 2 : 1;
	constexpr uint32_t NIMG = seg_images(W, 0);
	constexpr uint32_t LBC = CH < 2 ? 0u : NIMG - 1u; // as encode_kernel without a model
	constexpr uint32_t RW = EPT * W / 16u;
	constexpr bool EXT_HDR = !(PRE == PRE_NONE && ENC == ENC_RAW);
	constexpr uint32_t HDR_BITS = EXT_HDR ? 176u : 128u;
	extern __shared__ __attribute__((aligned(16))) uint32_t L_dyn[];
	const uint32_t IMGW = a.img_words + 4u;
	__shared__ uint32_t s_wsum[CH][EWG / 64];
	__shared__ uint32_t s_misc[8];
	__shared__ __attribute__((aligned(16))) uint2 s_rice[20];

	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);

	// ---- the front: this block's descriptor, one scalar load (glc: the host
	// rewrites the table between launches) ---------------------------------
	typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
	u32x8 d;
	{
		const uint64_t *dp = lb_sptr(reinterpret_cast<const uint64_t *>(t.desc + blockIdx.x));
		asm volatile("s_load_dwordx8 %0, %1, 0x0 glc\n\t"
			     "s_waitcnt lgkmcnt(0)"
			     : "=&s"(d)
			     : "s"(dp)
			     : "memory");
	}
	const uint8_t *fsrc = reinterpret_cast<const uint8_t *>((uintptr_t)(((uint64_t)d[1] << 32) | d[0]));
	const uint32_t n = d[2], sif = d[3], frame = d[4];
	const uint32_t gseg = d[5] + sif; // granule slot: frame-major
	const bool is_first = sif == 0u;
	const bool is_last = (uint64_t)(sif + 1u) * SEGN >= n;
	const bool src_al = ((uintptr_t)fsrc & 15u) == 0;

	// ---- phase 0: issue every load of the segment -----------------------
	uint32_t firstc[CH];
	uint4 raw[CH][RW];
	uint32_t prevld[CH];
#pragma unroll
	for (uint32_t c = 0; c < CH; c++) {
		firstc[c] = sif * SEGN + c * AIRS_SEG + tid * EPT;
		const bool full = firstc[c] + EPT <= n;
		if (full && src_al) {
			const uint4 *p = reinterpret_cast<const uint4 *>(fsrc + (size_t)firstc[c] * W);
#pragma unroll
			for (uint32_t q = 0; q < RW; q++)
				raw[c][q] = p[q];
		}
		prevld[c] = 0u;
		if (PRE == PRE_DIFF && lane == 0u && firstc[c] != 0u && firstc[c] <= n)
			prevld[c] = W == 2 ? (uint32_t)reinterpret_cast<const uint16_t *>(fsrc)[firstc[c] - 1u]
					   : reinterpret_cast<const uint32_t *>(fsrc)[firstc[c] - 1u] & 0xFFFFu;
	}
	// the frame's own fields, while the samples are in flight
	uint8_t *fdst = a.dst + t.dst_off[frame];
	const uint32_t cap = __builtin_amdgcn_readfirstlane(t.caps[frame]);

	// zero the LDS chunk images
	{
		uint4 *L4 = reinterpret_cast<uint4 *>(L_dyn);
		for (uint32_t i = tid; i < NIMG * IMGW / 4u; i += EWG)
			L4[i] = make_uint4(0u, 0u, 0u, 0u);
	}

	const uint32_t gpar = a.g;
	const Coder cd = make_coder<ENC>(ENC == ENC_RAW ? 1u : gpar, a.outlier_param);

	// ---- phase 1: residuals, mapped values, code lengths ------------------
	const bool fastk = ENC == ENC_ZERO && RICE && cd.k <= 11u;
	if (fastk && tid < 18u)
		s_rice[tid] = rice_table_entry(tid, cd.k);
	uint32_t mp[CH][EPT / 2];
	uint32_t mq[CH][EPT / 2];
	uint32_t T[CH], nv[CH];
#pragma unroll
	for (uint32_t c = 0; c < CH; c++) {
		const uint32_t first = firstc[c];
		nv[c] = first >= n ? 0u : min(n - first, (uint32_t)EPT);
		uint32_t w[EPT / 2];
		if (nv[c] == EPT && src_al) {
			if (W == 2) {
#pragma unroll
				for (uint32_t q = 0; q < RW; q++) {
					w[4 * q] = raw[c][q].x;
					w[4 * q + 1] = raw[c][q].y;
					w[4 * q + 2] = raw[c][q].z;
					w[4 * q + 3] = raw[c][q].w;
				}
			} else {
#pragma unroll
				for (uint32_t q = 0; q < RW; q++) {
					w[2 * q] = __builtin_amdgcn_perm(raw[c][q].y, raw[c][q].x, 0x05040100u);
					w[2 * q + 1] = __builtin_amdgcn_perm(raw[c][q].w, raw[c][q].z, 0x05040100u);
				}
			}
		} else {
#pragma unroll
			for (uint32_t j = 0; j < EPT / 2; j++) {
				uint32_t x2[2];
#pragma unroll
				for (uint32_t h = 0; h < 2; h++) {
					const uint32_t i = first + 2 * j + h;
					x2[h] = i < n ? (W == 2 ? (uint32_t)reinterpret_cast<const uint16_t *>(fsrc)[i]
								: reinterpret_cast<const uint32_t *>(fsrc)[i] & 0xFFFFu)
						      : 0u;
				}
				w[j] = x2[0] | x2[1] << 16;
			}
		}
		uint32_t wprev = 0u;
		if (PRE == PRE_DIFF) {
			wprev = __shfl_up(w[EPT / 2 - 1], 1, 64);
			if (lane == 0u)
				wprev = prevld[c] << 16;
		}
#pragma unroll
		for (uint32_t j = 0; j < EPT / 2; j++) {
			uint32_t u;
			if (PRE == PRE_DIFF)
				u = unpk(pk(w[j]) - pk(__builtin_amdgcn_alignbit(w[j], j ? w[j - 1] : wprev, 16)));
			else
				u = w[j];
			mp[c][j] = ENC == ENC_RAW ? u : zigzag_pk(u);
		}
		// code lengths of the chunk and, on the Rice/ZERO table path, the table
		// offsets of its samples
		uint32_t tl = 0u;
		if (fastk && nv[c] == EPT) {
			u16x2 acc = (u16x2)(0);
#pragma unroll
			for (uint32_t j = 0; j < EPT / 2; j++) {
				const u16x2 v = __builtin_elementwise_add_sat(pk(mp[c][j]), (u16x2)(1));
				const u16x2 q = v >> (u16x2)((unsigned short)cd.k);
				acc += __builtin_elementwise_min(q, (u16x2)(16));
				mq[c][j] = unpk(__builtin_elementwise_min(q, (u16x2)(17)) << (u16x2)(3));
			}
			tl = EPT * (cd.k + 1u) + (unpk(acc) & 0xFFFFu) + (unpk(acc) >> 16);
		} else {
#pragma unroll
			for (uint32_t j = 0; j < EPT; j++)
				tl += j < nv[c] ? len_from_m<ENC, RICE>(half16(mp[c][j >> 1], j & 1u), cd) : 0u;
#pragma unroll
			for (uint32_t j = 0; j < EPT / 2; j++)
				mq[c][j] = 0u;
		}
		T[c] = tl;
		// opaque, as in encode_kernel: keeps phase 1's intermediates from
		// living on into phase 2
#pragma unroll
		for (uint32_t i = 0; i < EPT / 2; i++)
			asm volatile("" : "+v"(mp[c][i]));
#pragma unroll
		for (uint32_t i = 0; i < EPT / 2; i++)
			asm volatile("" : "+v"(mq[c][i]));
	}

	// ---- per-chunk block scans --------------------------------------------
	uint32_t inc[CH];
#pragma unroll
	for (uint32_t c = 0; c < CH; c++) {
		inc[c] = wave_incl_scan(T[c]);
		if (lane == 63u)
			s_wsum[c][wid] = inc[c];
	}
	LbWin lbw = {0ull, 0ull};
	__syncthreads(); // B1: wave totals visible (and the images zeroed)
	uint32_t excl[CH], tot[CH], base[CH];
	uint32_t A = 0u;
#pragma unroll
	for (uint32_t c = 0; c < CH; c++) {
		uint32_t woff = 0u, tt = 0u;
#pragma unroll
		for (uint32_t w = 0; w < EWG / 64; w++) {
			const uint32_t v = s_wsum[c][w];
			woff += w < wid ? v : 0u;
			tt += v;
		}
		excl[c] = woff + inc[c] - T[c];
		tot[c] = __builtin_amdgcn_readfirstlane(tt);
		base[c] = A;
		A += tt;
	}
	const uint32_t first_seg = gseg - sif;
	if (wid == 0) {
		if (lane == 0) {
			const uint64_t tag = ((uint64_t)a.epoch << 1) | (is_first ? 1u : 0u);
			gran_store(&a.agg[gseg], (tag << 32) | (is_first ? HDR_BITS + A : A));
		}
		if (LBC == 0 && !is_first)
			lbw = lb_prefetch(a, gseg, first_seg, lane);
	}
	// ---- the segment's last 32 bits (the last wave rebuilds its last chunk) --
	// (a segment that is not the frame's last is whole: nv[CH - 1] == EPT)
	if (!is_last && wid == EWG / 64 - 1) {
		uint64_t acc = 0u;
		if (fastk) {
			const char *tab = reinterpret_cast<const char *>(s_rice);
			auto pair = [&](uint32_t j) {
				const u16x2 qa = pk(mq[CH - 1][j]);
#pragma unroll
				for (uint32_t h = 0; h < 2; h++) {
					const uint2 e = *reinterpret_cast<const uint2 *>(tab + half16(unpk(qa), h));
					acc = (acc << e.y) | (half16(mp[CH - 1][j], h) + e.x);
				}
			};
			if (EPT >= 16 && cd.k >= 3u) {
#pragma unroll
				for (uint32_t j = EPT / 4; j < EPT / 2; j++)
					pair(j);
			} else {
#pragma unroll
				for (uint32_t j = 0; j < EPT / 2; j++)
					pair(j);
			}
		} else {
#pragma unroll
			for (uint32_t j = 0; j < EPT; j++) {
				const uint32_t m = (mp[CH - 1][j >> 1] >> (16u * (j & 1u))) & 0xFFFFu;
				uint32_t c1, l1, c2, l2;
				code_from_m<ENC, RICE>(m, cd, c1, l1, c2, l2);
				acc = (acc << l1) | c1;
				if (NPIECE == 2)
					acc = (acc << l2) | c2;
			}
		}
		uint32_t v = (uint32_t)acc, tb = min(T[CH - 1], 32u);
#pragma unroll
		for (uint32_t dd = 1; dd <= 2; dd <<= 1) {
			const uint32_t va = __shfl_up(v, dd, 64), ta = __shfl_up(tb, dd, 64);
			if (lane >= dd && tb < 32u) {
				v = (va << tb) | v;
				tb = min(ta + tb, 32u);
			}
		}
		if (lane == 63u)
			gran_store(&a.tail[gseg], ((uint64_t)a.epoch << 32) | v);
	}

	uint32_t last_ne = 0u; // last non-empty chunk
#pragma unroll
	for (uint32_t c = 0; c < CH; c++)
		last_ne = tot[c] ? c : last_ne;

	const __amdgpu_buffer_rsrc_t dst_rsrc = __builtin_amdgcn_make_buffer_rsrc(fdst, 0, (int)(cap & ~3u), 0x00020000);
	uint32_t P = 0u;
	uint32_t pred_c = 0u;
	const uint32_t tot_first = tot[0];

	// one chunk image to its frame bit offset, clipped to the frame's capacity
	// by the buffer descriptor's range (encode_kernel's store_chunk)
	auto store_chunk = [&](const uint32_t *Lx, uint32_t basex, uint32_t totx, uint32_t predx, bool finalx) {
		if (!totx)
			return;
		const uint32_t Pc = P + basex;
		const uint32_t r = Pc & 31u, g0 = Pc >> 5;
		const uint32_t endbit = Pc + totx;
		const uint32_t J = ((endbit - 1u) >> 5) - g0;
		const uint32_t nfull = (endbit & 31u) == 0u ? J + 1u : J;
		const lds_u32 *Ll = reinterpret_cast<const lds_u32 *>((uintptr_t)Lx);
		const uint32_t nquad = nfull >> 2;
		for (uint32_t p = tid; p < nquad; p += EWG) {
			const uint32_t j = 4u * p;
			const u32x4 w = *reinterpret_cast<const __attribute__((address_space(3))) u32x4 *>(Ll + j);
			const uint32_t hi = j ? Ll[j - 1u] : predx;
			u32x4 o;
			o.x = bswap32(__builtin_amdgcn_alignbit(hi, w.x, r));
			o.y = bswap32(__builtin_amdgcn_alignbit(w.x, w.y, r));
			o.z = bswap32(__builtin_amdgcn_alignbit(w.y, w.z, r));
			o.w = bswap32(__builtin_amdgcn_alignbit(w.z, w.w, r));
			__builtin_amdgcn_raw_buffer_store_b128(o, dst_rsrc, (int)(4u * (g0 + j)), 0, 0);
		}
		const uint32_t rr = (tid - nquad) & (EWG - 1u);
		if (rr < (nfull & 3u)) {
			const uint32_t j = 4u * nquad + rr;
			const uint32_t hi = j ? Ll[j - 1u] : predx;
			const uint32_t v = __builtin_amdgcn_alignbit(hi, Ll[j], r);
			__builtin_amdgcn_raw_buffer_store_b32(bswap32(v), dst_rsrc, (int)(4u * (g0 + j)), 0, 0);
		}
		if (finalx && nfull == J && tid == 0) {
			const uint32_t hi = J ? Lx[J - 1u] : predx;
			const uint32_t v = __builtin_amdgcn_alignbit(hi, Lx[J], r);
			const uint32_t gw = g0 + J;
			const uint32_t nbytes = ((endbit & 31u) + 7u) >> 3;
			for (uint32_t b = 0; b < nbytes; b++)
				if (4u * gw + b < cap)
					fdst[4u * gw + b] = (uint8_t)(v >> (24u - 8u * b));
		}
	};

	// ---- phase 2: chunk by chunk: codewords -> LDS image -> HBM -----------
	__builtin_amdgcn_s_setprio(1);
	uint32_t tot_m3 = 0u, tot_m2 = 0u, tot_m1 = 0u;
	uint32_t pred_1 = 0u, pred_2 = 0u;
#pragma unroll
	for (uint32_t c = 0; c < CH; c++) {
		uint32_t *Lc = L_dyn + (c % NIMG) * IMGW + 4u;
		if (LBC >= 1 && c == LBC + 1u && c >= NIMG)
			__syncthreads(); // chunk 0's image was stored (late) after the last barrier
		if (c >= NIMG) {
			const uint32_t nw = (max(NIMG == 2 ? tot_m2 : tot_m3, tot[0]) + 31u) >> 5;
			for (uint32_t i = tid; i <= nw; i += EWG)
				Lc[i] = 0u;
			__syncthreads();
		}
		if (LBC >= 1 && c == LBC && wid == 0 && !is_first && sif < AIRS_LB_SCALAR_N)
			lbw = lb_prefetch(a, gseg, first_seg, lane);
		{
			Packer pk1;
			pk1.init(Lc, excl[0]);
			if (fastk && nv[0] == EPT) {
				const char *tab = reinterpret_cast<const char *>(s_rice);
#pragma unroll
				for (uint32_t hb = 0; hb < 2; hb++) {
					uint2 te[EPT / 2];
#pragma unroll
					for (uint32_t jj = 0; jj < EPT / 4; jj++) {
						const uint32_t j = hb * (EPT / 4) + jj;
						const u16x2 qa = pk(mq[0][j]);
#pragma unroll
						for (uint32_t h = 0; h < 2; h++)
							te[2 * jj + h] = *reinterpret_cast<const uint2 *>(tab + half16(unpk(qa), h));
					}
					uint32_t mxl = 0u;
#pragma unroll
					for (uint32_t i = 0; i < EPT / 2; i += 2)
						mxl = max(mxl, te[i].y + te[i + 1].y);
					if (__ballot(mxl > 32u) == 0ull) {
#pragma unroll
						for (uint32_t i = 0; i < EPT / 2; i += 2) {
							const uint32_t j = hb * (EPT / 2) + i;
							const uint32_t cwa = (mp[0][j >> 1] & 0xFFFFu) + te[i].x;
							const uint32_t cwb = (mp[0][j >> 1] >> 16) + te[i + 1].x;
							pk1.put((cwa << te[i + 1].y) | cwb, te[i].y + te[i + 1].y);
						}
					} else {
#pragma unroll
						for (uint32_t i = 0; i < EPT / 2; i += 2) {
							const uint32_t j = hb * (EPT / 2) + i;
							pk1.put((mp[0][j >> 1] & 0xFFFFu) + te[i].x, te[i].y);
							pk1.put((mp[0][j >> 1] >> 16) + te[i + 1].x, te[i + 1].y);
						}
					}
				}
			} else {
#pragma unroll
				for (uint32_t j = 0; j < EPT; j++) {
					const uint32_t m = half16(mp[0][j >> 1], j & 1u);
					uint32_t c1, l1, c2, l2;
					code_from_m<ENC, RICE>(m, cd, c1, l1, c2, l2);
					const bool ok = j < nv[0];
					l1 = ok ? l1 : 0u;
					pk1.put(ok ? c1 : 0u, l1);
					if (NPIECE == 2) {
						l2 = ok ? l2 : 0u;
						pk1.put(ok ? c2 : 0u, l2);
					}
				}
			}
			pk1.flush();
		}
		__syncthreads();
		uint32_t pred_next = 0u; // last 32 bits of this chunk, for chunk c+1 (tid 0)
		if (c + 1u < CH && tid == 0 && tot[0] >= 32u) {
			const uint32_t s0 = tot[0] - 32u, q = s0 >> 5, sh = s0 & 31u;
			pred_next = sh ? (Lc[q] << sh) | (Lc[q + 1] >> (32u - sh)) : Lc[q];
		}

		if (c == LBC) {
			// ---- decoupled look-back (wave 0), overlapped with the packing ----
			if (wid == 0) {
				uint32_t Pw = HDR_BITS, pred = 0u;
				if (is_first) {
					// header bytes 20-21 share the first payload dword of a 22-byte header
					pred = (EXT_HDR && ENC != ENC_RAW) ? (cd.outlier & 0xFFFFu) : 0u;
				} else {
					if (LBC >= 1 && sif >= AIRS_LB_SCALAR_N)
						lbw = lb_scalar(a, gseg, lane, 0ull);
					const uint2 pp = lb_resolve(a, gseg, sif, lane, lbw.gv, lbw.tv, 1u);
					Pw = pp.x;
					pred = pp.y;
					if (lane == 0)
						gran_store(&a.agg[gseg], ((((uint64_t)a.epoch << 1) | 1u) << 32) | (Pw + A));
				}
				if (lane == 0) {
					s_misc[1] = Pw;
					s_misc[2] = pred;
				}
			}
			__syncthreads();
			P = __builtin_amdgcn_readfirstlane(s_misc[1]);
			const uint32_t seg_pred = __builtin_amdgcn_readfirstlane(s_misc[2]);
			if (LBC == 0)
				pred_c = seg_pred;
			else if (tot_first)
				store_chunk(L_dyn + 4u, 0u, tot_first, seg_pred, is_last && last_ne == 0u);
			if (LBC == 2)
				store_chunk(L_dyn + IMGW + 4u, tot_first, tot_m1, pred_1, is_last && last_ne == 1u);
			if (LBC == 3) {
				store_chunk(L_dyn + IMGW + 4u, tot_first, tot_m2, pred_1, is_last && last_ne == 1u);
				store_chunk(L_dyn + 2u * IMGW + 4u, tot_first + tot_m2, tot_m1, pred_2,
					    is_last && last_ne == 2u);
			}
		}

		if (c >= LBC)
			store_chunk(Lc, base[0], tot[0], pred_c, is_last && c == last_ne);

		if (c == 0)
			pred_1 = pred_next;
		if (c == 1)
			pred_2 = pred_next;
		pred_c = pred_next;
		// rotate the per-chunk state
		tot_m3 = tot_m2;
		tot_m2 = tot_m1;
		tot_m1 = tot[0];
#pragma unroll
		for (uint32_t k = 0; k + 1 < CH; k++) {
#pragma unroll
			for (uint32_t i = 0; i < EPT / 2; i++) {
				mp[k][i] = mp[k + 1][i];
				mq[k][i] = mq[k + 1][i];
			}
			nv[k] = nv[k + 1];
			excl[k] = excl[k + 1];
			tot[k] = tot[k + 1];
			base[k] = base[k + 1];
		}
	}

	// ---- frame epilogue: checksum (when the launch has one), header, status --
	if (is_last && tid == 0) {
		const uint32_t payload_bytes = (P + A + 7u) >> 3;
		const uint32_t size = payload_bytes + (t.checksums ? 4u : 0u);
		if (t.checksums) { // as encode_kernel's epilogue: big-endian, clipped to the capacity
			const uint32_t ck = t.checksums[frame];
			for (uint32_t b = 0; b < 4u; b++)
				if (payload_bytes + b < cap)
					fdst[payload_bytes + b] = (uint8_t)(ck >> (24u - 8u * b));
		}
		uint32_t h[5];
		header_words(h, size, 2u * n, t.ids[frame], t.seqs[frame], PRE, t.checksums ? 1u : 0u, ENC, 0u,
			     ENC == ENC_RAW ? 0u : gpar, ENC == ENC_RAW ? 0u : cd.outlier);
		const uint32_t hwords = EXT_HDR ? 5u : 4u;
		if (((uintptr_t)fdst & 7u) == 0u && cap >= 4u * hwords) {
			*reinterpret_cast<uint2 *>(fdst) = make_uint2(bswap32(h[0]), bswap32(h[1]));
			*reinterpret_cast<uint2 *>(fdst + 8) = make_uint2(bswap32(h[2]), bswap32(h[3]));
			if (hwords == 5u)
				*reinterpret_cast<uint32_t *>(fdst + 16) = bswap32(h[4]);
		} else {
#pragma unroll
			for (uint32_t w = 0; w < 5u; w++)
				if (w < hwords && 4u * w + 4u <= cap)
					*reinterpret_cast<uint32_t *>(fdst + 4u * w) = bswap32(h[w]);
		}
		uint32_t st = size;
		if (size > cap)
			st = ERRV(E_DST_TOO_SMALL);
		else if (size > 0xFFFFFFu)
			st = ERRV(E_HDR_CMP_SIZE_TOO_LARGE);
		a.status[frame] = st;
	}
}

template <int W, int PRE, int ENC, bool RICE>
static void ragged_go(const KArgs &k, const RaggedTabs &t, uint32_t grid, hipStream_t s)
{
	const size_t lds = (size_t)seg_images(W, 0) * (k.img_words + 4u) * 4u;
	hipLaunchKernelGGL((ragged_kernel<W, PRE, ENC, RICE>), dim3(grid), dim3(EWG), lds, s, k, t);
}

template <int W, int PRE>
static void ragged_enc(const KArgs &k, const RaggedTabs &t, uint32_t enc, bool rice, uint32_t grid, hipStream_t s)
{
	switch (enc) {
	case ENC_RAW:
		ragged_go<W, PRE, ENC_RAW, true>(k, t, grid, s);
		break;
	case ENC_ZERO:
		if (rice)
			ragged_go<W, PRE, ENC_ZERO, true>(k, t, grid, s);
		else
			ragged_go<W, PRE, ENC_ZERO, false>(k, t, grid, s);
		break;
	default:
		if (rice)
			ragged_go<W, PRE, ENC_MULTI, true>(k, t, grid, s);
		else
			ragged_go<W, PRE, ENC_MULTI, false>(k, t, grid, s);
		break;
	}
}

uint32_t ragged_segn(uint32_t sample_bytes)
{
	return seg_chunks(sample_bytes == 4 ? 4 : 2, 0) * AIRS_SEG;
}

void ragged_encode(const KArgs &k, const RaggedTabs &t, uint32_t sample_bytes, uint32_t pre, uint32_t enc, bool rice,
		   uint32_t grid, hipStream_t s)
{
	if (sample_bytes == 2) {
		if (pre == PRE_DIFF)
			ragged_enc<2, PRE_DIFF>(k, t, enc, rice, grid, s);
		else
			ragged_enc<2, PRE_NONE>(k, t, enc, rice, grid, s);
	} else {
		if (pre == PRE_DIFF)
			ragged_enc<4, PRE_DIFF>(k, t, enc, rice, grid, s);
		else
			ragged_enc<4, PRE_NONE>(k, t, enc, rice, grid, s);
	}
}

} // namespace airs
