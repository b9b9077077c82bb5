// fitsin.hip -- FITS image data units in device memory, as they lie in the file, into native float32 frames (tp_fits_unpack) and their
// DATASUM word sum (tp_fits_datasum): what astropy's `hdu.data[r0:r1, c0:c1]` with `dtype='float32'` does on the host in the reference
// (io.py:46-48, :80-82).  The decisions -- BITPIX, window, vector or scalar rows, the float64 rounding, the carry fold -- are the rules
// of fits_rules.h; this file is their parallel plumbing.
//
// Traffic per data unit of a TESS FFI (2078 x 2136 float32 = 17 755 200 bytes with its padding, window 2048 x 2048):
//   tp_fits_datasum reads the whole unit once                     17.8 MB
//   tp_fits_unpack reads the window and writes it                 16.8 MB + 16.8 MB
// two passes, 51.3 MB per unit, 102.7 MB per frame (image and uncertainty).  One fused pass over the full rows would save the second
// read of the window (34 MB per frame), which comes out of the 256 MiB last-level cache anyway: the unit was written there by the
// transfer a moment before.  Two entries keep the checksum optional and the unpacker free of the bytes outside its window.
#include "common.h"
#include "fits_rules.h"

using namespace tp_fits;

namespace {

// one value of the file at p as the bits of the float32 it becomes
template <int ITEM> __device__ inline uint32_t value_bits(const unsigned char* p)
{
	if (ITEM == 4) return bswap32(*reinterpret_cast<const uint32_t*>(p));
	const uint2 w = *reinterpret_cast<const uint2*>(p);
	return f64_to_f32_bits(((uint64_t)bswap32(w.x) << 32) | bswap32(w.y));
}
// four values from a 16-byte boundary
template <int ITEM> __device__ inline uint4 group_bits(const unsigned char* p)
{
	const uint4 a = *reinterpret_cast<const uint4*>(p);
	if (ITEM == 4) return make_uint4(bswap32(a.x), bswap32(a.y), bswap32(a.z), bswap32(a.w));
	const uint4 b = *reinterpret_cast<const uint4*>(p + 16);
	return make_uint4(f64_to_f32_bits(((uint64_t)bswap32(a.x) << 32) | bswap32(a.y)), f64_to_f32_bits(((uint64_t)bswap32(a.z) << 32) | bswap32(a.w)),
		f64_to_f32_bits(((uint64_t)bswap32(b.x) << 32) | bswap32(b.y)), f64_to_f32_bits(((uint64_t)bswap32(b.z) << 32) | bswap32(b.w)));
}

// Vector rows: thread g of a row moves group g of the body (one 16-byte store, one or two 16-byte loads: a wavefront stores 1 KiB
// in a line); the first threads of the row's first block also move the head and the tail.  Rows stride over gridDim.y.
template <int ITEM> __global__ void __launch_bounds__(kThreads) tp_fits_unpack_kernel(const unsigned char* __restrict__ raw, int64_t naxis1, int64_t row0, int64_t col0,
	int64_t rows, RowPlan plan, uint32_t* __restrict__ out, int64_t pitch)
{
	const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
	for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
		const unsigned char* src = raw + ((row0 + r) * naxis1 + col0) * ITEM;
		uint32_t* dst = out + r * pitch;
		if (g < plan.body4)
			*reinterpret_cast<uint4*>(dst + plan.head + 4 * g) = group_bits<ITEM>(src + (plan.head + 4 * g) * ITEM);
		if (blockIdx.x == 0) {
			const int64_t t = threadIdx.x;
			if (t < plan.head) dst[t] = value_bits<ITEM>(src + t * ITEM);
			const int64_t c = plan.head + 4 * plan.body4 + t;
			if (t < plan.tail) dst[c] = value_bits<ITEM>(src + c * ITEM);
		}
	}
}

// Scalar rows: one value per thread
template <int ITEM> __global__ void __launch_bounds__(kThreads) tp_fits_unpack_scalar_kernel(const unsigned char* __restrict__ raw, int64_t naxis1, int64_t row0, int64_t col0,
	int64_t rows, int64_t cols, uint32_t* __restrict__ out, int64_t pitch)
{
	const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
	if (c >= cols) return;
	for (int64_t r = blockIdx.y; r < rows; r += gridDim.y)
		out[r * pitch + c] = value_bits<ITEM>(raw + ((row0 + r) * naxis1 + col0 + c) * ITEM);
}

// The plain 64-bit sum of the big-endian words: n16 pieces of 16 bytes over the grid, the n_tail words after them by the first
// threads of block 0; a wavefront's sums meet by shuffles, a block's in LDS, the blocks' by one integer atomic each.
__global__ void __launch_bounds__(kThreads) tp_fits_datasum_kernel(const unsigned char* __restrict__ raw, uint64_t n16, int32_t n_tail, unsigned long long* __restrict__ sum)
{
	__shared__ unsigned long long part[kThreads / 64];
	const uint4* v = reinterpret_cast<const uint4*>(raw);
	unsigned long long s = 0;
	const uint64_t stride = (uint64_t)gridDim.x * kThreads;
	uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
	for (; i + (kSumUnroll - 1) * stride < n16; i += kSumUnroll * stride) {
		uint4 a[kSumUnroll];
#pragma unroll
		for (int k = 0; k < kSumUnroll; k++) a[k] = v[i + k * stride];
#pragma unroll
		for (int k = 0; k < kSumUnroll; k++) s += ((unsigned long long)bswap32(a[k].x) + bswap32(a[k].y)) + ((unsigned long long)bswap32(a[k].z) + bswap32(a[k].w));
	}
	for (; i < n16; i += stride) {
		const uint4 a = v[i];
		s += ((unsigned long long)bswap32(a.x) + bswap32(a.y)) + ((unsigned long long)bswap32(a.z) + bswap32(a.w));
	}
	if (blockIdx.x == 0 && (int)threadIdx.x < n_tail) s += bswap32(reinterpret_cast<const uint32_t*>(raw + n16 * 16)[threadIdx.x]);
	for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long b = 0;
		for (int w = 0; w < kThreads / 64; w++) b += part[w];
		atomicAdd(sum, b);
	}
}

__global__ void tp_fits_fold_kernel(unsigned long long* sum) { *sum = fold32(*sum); }

} // namespace

extern "C" int tp_fits_unpack(tp_ctx* ctx, const void* d_raw, int32_t bitpix, int32_t naxis1, int32_t naxis2, int32_t row0, int32_t col0, int32_t rows,
	int32_t cols, float* d_out, int64_t out_row_pitch)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const uint64_t raw_addr = reinterpret_cast<uintptr_t>(d_raw), out_addr = reinterpret_cast<uintptr_t>(d_out);
	const char* msg = unpack_check(raw_addr, bitpix, naxis1, naxis2, row0, col0, rows, cols, out_addr, out_row_pitch);
	TP_REQUIRE(ctx, msg == nullptr, msg);
	const int item = item_bytes(bitpix);
	const RowPlan plan = row_plan(raw_addr, item, naxis1, row0, col0, cols, out_addr, out_row_pitch);
	const unsigned char* raw = static_cast<const unsigned char*>(d_raw);
	uint32_t* out = reinterpret_cast<uint32_t*>(d_out);
	const unsigned gy = (unsigned)(rows < 65535 ? rows : 65535);
	if (plan.vec) {
		const dim3 grid((unsigned)((plan.body4 + kThreads - 1) / kThreads), gy);
		if (item == 4)
			TP_LAUNCH(ctx, TPK_FITS_UNPACK, tp_fits_unpack_kernel<4>, grid, dim3(kThreads), 0, raw, (int64_t)naxis1, (int64_t)row0, (int64_t)col0, (int64_t)rows, plan, out, out_row_pitch);
		else
			TP_LAUNCH(ctx, TPK_FITS_UNPACK, tp_fits_unpack_kernel<8>, grid, dim3(kThreads), 0, raw, (int64_t)naxis1, (int64_t)row0, (int64_t)col0, (int64_t)rows, plan, out, out_row_pitch);
		TP_LAUNCH_CHECK(ctx, "tp_fits_unpack_kernel");
	} else {
		const dim3 grid((unsigned)((cols + kThreads - 1) / kThreads), gy);
		if (item == 4)
			TP_LAUNCH(ctx, TPK_FITS_UNPACK_SCALAR, tp_fits_unpack_scalar_kernel<4>, grid, dim3(kThreads), 0, raw, (int64_t)naxis1, (int64_t)row0, (int64_t)col0, (int64_t)rows, (int64_t)cols, out, out_row_pitch);
		else
			TP_LAUNCH(ctx, TPK_FITS_UNPACK_SCALAR, tp_fits_unpack_scalar_kernel<8>, grid, dim3(kThreads), 0, raw, (int64_t)naxis1, (int64_t)row0, (int64_t)col0, (int64_t)rows, (int64_t)cols, out, out_row_pitch);
		TP_LAUNCH_CHECK(ctx, "tp_fits_unpack_scalar_kernel");
	}
	return TP_OK;
	TP_API_END(ctx)
}

extern "C" int tp_fits_datasum(tp_ctx* ctx, const void* d_raw, uint64_t nbytes, uint64_t* d_wordsum)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const char* msg = datasum_check(reinterpret_cast<uintptr_t>(d_raw), nbytes, reinterpret_cast<uintptr_t>(d_wordsum));
	TP_REQUIRE(ctx, msg == nullptr, msg);
	unsigned long long* sum = reinterpret_cast<unsigned long long*>(d_wordsum);
	TP_HIP(ctx, hipMemsetAsync(sum, 0, sizeof(unsigned long long), ctx->stream));
	if (nbytes == 0) return TP_OK;
	const uint64_t n16 = nbytes / 16;
	TP_LAUNCH(ctx, TPK_FITS_DATASUM, tp_fits_datasum_kernel, dim3((unsigned)sum_blocks(n16)), dim3(kThreads), 0, static_cast<const unsigned char*>(d_raw), n16,
		(int32_t)((nbytes % 16) / 4), sum);
	TP_LAUNCH_CHECK(ctx, "tp_fits_datasum_kernel");
	TP_LAUNCH(ctx, TPK_FITS_FOLD, tp_fits_fold_kernel, dim3(1), dim3(1), 0, sum);
	TP_LAUNCH_CHECK(ctx, "tp_fits_fold_kernel");
	return TP_OK;
	TP_API_END(ctx)
}
