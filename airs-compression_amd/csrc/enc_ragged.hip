// enc_ragged.hip -- ragged encode launches (cmp_gpu_compress_image with
// CMP_GPU_OPT_IMAGE_RAGGED): frames of different sizes in one
// launch.  The encode kernel (enc_kernel.h) in its ragged mode, compiled in its
// own translation unit.
//
// The mode is for launches without a model, IWT, fused Rice selection or
// payload-only stream.  A block reads one 32-byte descriptor (airs_ragged_desc)
// with a single scalar load before its sample loads: the frame's sample address
// and sample count, the block's segment of the frame, the frame's index in the
// piece and its first granule slot.  Destination offset, capacity, identifier,
// sequence number and checksum come from per-frame arrays (RaggedTabs, the
// kernel's second argument).  Phase 1, the packer, the look-back, the stores and
// the header are the kernel's own, not-FULL and without a model.
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

uint32_t ragged_segn(uint32_t sample_bytes)
{
	return seg_chunks(sample_bytes == 4 ? 4 : 2, 0) * AIRS_SEG;
}

void ragged_encode(const KArgs &k, const RaggedTabs &t, uint32_t sample_bytes, uint32_t pre, uint32_t enc, bool rice,
		   uint32_t grid, hipStream_t s)
{
	with_width_pre_coder(sample_bytes, pre, enc, rice, [&](auto w, auto p, auto e, auto r) {
		constexpr int W = w, PRE = p, ENC = e;
		constexpr bool RICE = r;
		const size_t lds = (size_t)seg_images(W, 0) * (k.img_words + 4u) * 4u;
		launch_segments(encode_kernel<W, PRE, ENC, RICE, 0, false, false, false, RaggedTabs>, k, grid, lds, s, t);
	});
}

} // namespace airs
