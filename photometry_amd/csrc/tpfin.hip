// tpfin.hip -- the image columns of a target pixel file's PIXELS table, in device memory as they lie in the file, into float32 stamp
// cubes (tp_tpf_unpack): what BasePhotometry._load_cube does on the host in the reference, `cube[:, :, k] = data[field][k]` for every
// table row k (BasePhotometry.py:720-751).  In the file a row is one cadence and holds all its pixels, big-endian; in a cube
// [n_pix][t_pitch] a pixel's series is contiguous.  The work is a byte swap and a transposition.  The decisions -- argument checks,
// tile geometry, LDS index, pad range -- are the rules of tpf_rules.h; this file is their parallel plumbing.
//
// A workgroup of 256 threads owns a tile of 64 cadences x 64 pixels of one column (the columns lie on blockIdx.z).  Loading, a
// wavefront reads 64 consecutive dwords of a table row (256 bytes, coalesced; rows are in general only 4-byte aligned -- an 11 x 12
// stamp has rows of 2668 bytes -- so the loads are dwords), swaps them and writes them to row tt of an LDS tile.  After a barrier a
// wavefront reads column pp of the tile and stores it with lane = cadence: 256 contiguous bytes of the pixel's series.
//
// The LDS tile has a pitch of 65 dwords.  ds_write_b32 and ds_read_b32 bank on (byte address / 4) mod 32, and only the lanes of
// one 32-lane half of a wavefront conflict with each other.  The writes of a wavefront are 64 consecutive dwords: 32 different
// banks per half.  The transposed reads are 65 dwords apart, and 65 = 1 (mod 32): lane l of a half reads bank (base + l) mod 32,
// again 32 different banks.  Both sides are free of conflicts; with a pitch of 64 every lane of the read would meet bank `pp`.
//
// Traffic per file of a 2-minute target (11 x 11 pixels, 19 000 rows of 2.4 kB; FLUX, FLUX_ERR, FLUX_BKG): 3 x 9.2 MB read out of
// the 46 MB table, 3 x 9.2 MB written.  The cadences behind the last one up to t_pitch are written as 0.0 here, so a cube needs no memset.
#include "common.h"
#include "tpf_rules.h"

using namespace tp_tpf;

namespace {

struct TpfColumns {
	int64_t offset[kMaxCols];
	uint32_t* out[kMaxCols];
};

__global__ void __launch_bounds__(kThreads) tp_tpf_unpack_kernel(const unsigned char* __restrict__ table, int64_t row_bytes, const int32_t* __restrict__ rows, int64_t T,
	TpfColumns cols, int64_t n_pix, int64_t t_pitch)
{
	__shared__ uint32_t tile[kLdsWords];
	const int64_t t0 = (int64_t)blockIdx.x * kTileT, p0 = (int64_t)blockIdx.y * kTileP;
	const int64_t col_offset = cols.offset[blockIdx.z];
	uint32_t* __restrict__ out = cols.out[blockIdx.z];
	const int thread = threadIdx.x;

	if (t0 < T) {                                          // (a tile of pad cadences alone has nothing to load)
#pragma unroll
		for (int step = 0; step < kSteps; step++) {
			const TileElem e = load_elem(thread, step);
			const int64_t t = t0 + e.tt, pixel = p0 + e.pp;
			if (t < T && pixel < n_pix) {
				const int64_t row = rows ? (int64_t)rows[t] : t;
				tile[lds_index(e.tt, e.pp)] = bswap32(*reinterpret_cast<const uint32_t*>(table + src_byte(row, row_bytes, col_offset, pixel)));
			}
		}
	}
	__syncthreads();
#pragma unroll
	for (int step = 0; step < kSteps; step++) {
		const TileElem e = store_elem(thread, step);
		const int64_t t = t0 + e.tt, pixel = p0 + e.pp;
		if (pixel >= n_pix) continue;
		const int kind = store_kind(t, T, t_pitch);
		if (kind == kStoreValue) out[dst_index(pixel, t, t_pitch)] = tile[lds_index(e.tt, e.pp)];
		else if (kind == kStorePad) out[dst_index(pixel, t, t_pitch)] = 0u;
	}
}

} // namespace

extern "C" int tp_tpf_unpack(tp_ctx* ctx, const void* d_table, int64_t row_bytes, int64_t n_rows, const int32_t* h_rows, int64_t T, int32_t n_cols,
	const int64_t* h_col_offsets, int64_t n_pix, float* const* h_d_out, int64_t t_pitch)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	uint64_t out_addrs[kMaxCols] = {0, 0, 0, 0};
	if (h_d_out != nullptr && n_cols >= 1 && n_cols <= kMaxCols)
		for (int c = 0; c < n_cols; c++) out_addrs[c] = reinterpret_cast<uintptr_t>(h_d_out[c]);
	const char* msg = unpack_check(reinterpret_cast<uintptr_t>(d_table), row_bytes, n_rows, h_rows, T, n_cols, h_col_offsets, n_pix, h_d_out ? out_addrs : nullptr, t_pitch);
	TP_REQUIRE(ctx, msg == nullptr, msg);
	TpfColumns cols;
	for (int c = 0; c < kMaxCols; c++) {
		cols.offset[c] = c < n_cols ? h_col_offsets[c] : 0;
		cols.out[c] = c < n_cols ? reinterpret_cast<uint32_t*>(h_d_out[c]) : nullptr;
	}
	// the kept rows go up by the library's small-transfer path; their block returns to the context's cache behind the kernel
	void* d_rows = nullptr;
	if (h_rows != nullptr) {
		int rc = tp_malloc(ctx, (uint64_t)T * sizeof(int32_t), &d_rows);
		if (rc != TP_OK) return rc;
		rc = tp_memcpy_h2d(ctx, d_rows, h_rows, (uint64_t)T * sizeof(int32_t));
		if (rc != TP_OK) { (void)tp_free(ctx, d_rows); return rc; }
	}
	const dim3 grid((unsigned)grid_t(t_pitch), (unsigned)grid_p(n_pix), (unsigned)n_cols);
	TP_LAUNCH(ctx, TPK_TPF_UNPACK, tp_tpf_unpack_kernel, grid, dim3(kThreads), 0, static_cast<const unsigned char*>(d_table), row_bytes,
		static_cast<const int32_t*>(d_rows), T, cols, n_pix, t_pitch);
	const hipError_t launched = hipGetLastError();
	if (d_rows != nullptr) (void)tp_free(ctx, d_rows);
	if (launched != hipSuccess) return ctx->fail(TP_ERR_HIP, "tp_tpf_unpack_kernel", launched);
	return TP_OK;
	TP_API_END(ctx)
}
