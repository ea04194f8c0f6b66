// enc_stream.hip -- payload-only streams (cmp_gpu_encode_stream): the
// encode kernel in STREAM mode, compiled in its own translation unit.
//
// A stream is one frame without header, checksum or 24-bit size limit: the
// reference's encoder loop as compress_engine runs it for the payload
// (preprocess.c NONE/DIFF -> cmp_encoder_encode_s16 encoder.c:327-378 ->
// bitstream_writer.h:124-158, bitstream_flush :205-227), over up to
// AIRS_STREAM_MAX samples.  Its segments form ONE look-back chain (16 Ki
// segments for 256 Mi samples); its look-back reads one window of 64
// granules per round, like a frame's (lb_resolve, enc_common.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "enc_kernel.h"

namespace airs {

uint32_t stream_segn(uint32_t sample_bytes)
{
	return seg_chunks(sample_bytes == 4 ? 4 : 2, 0) * AIRS_SEG;
}

void stream_encode(const KArgs &k, uint32_t sample_bytes, uint32_t pre, uint32_t enc, bool rice, bool full,
		   uint32_t grid, hipStream_t s)
{
	with_width_pre_coder(sample_bytes, pre, enc, rice, [&](auto w, auto p, auto e, auto r) {
		constexpr int W = w, PRE = p, ENC = e;
		constexpr bool RICE = r;
		const size_t lds = (size_t)seg_images(W, 0) * (k.img_words + 4u) * 4u;
		if (full)
			launch_segments(encode_kernel<W, PRE, ENC, RICE, 0, true, false, true>, k, grid, lds, s);
		else
			launch_segments(encode_kernel<W, PRE, ENC, RICE, 0, false, false, true>, k, grid, lds, s);
	});
}

} // namespace airs
