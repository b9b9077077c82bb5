// inflate.hip -- batched DEFLATE decoding (RFC 1951) on the device: the raw deflate streams of a call become their bytes, each in a
// slot of its own, with status, bytes produced, bytes consumed and the CRC-32 of the bytes produced (tp_inflate).  What is decoded
// how -- bit reader, block headers, code tables, symbol chain, window, flush, CRC, statuses -- is the rules of inflate_rules.h; this
// file is the launch: one wavefront (a workgroup of 64) owns a stream from its first load to its last store.
//
// tp_inflate_kernel: inflate_stream of the rules on the stream's Lds (39.6 KiB: four wavefronts per CU).  The symbol chain is the same
// on every lane and held in scalar registers (what LDS returns goes through readfirstlane); the pieces the lanes share -- input refill,
// table build, stored copy, match copy, flush with the slice CRCs -- run between two barriers of the one-wavefront workgroup, which
// cost a wait for the LDS counter.  A stream writes its slot and its four results and nothing else, whatever its bytes hold.
#include "common.h"
#include "inflate_rules.h"

using namespace tp_inflate_rules;

namespace {

__global__ void __launch_bounds__(kLanes) tp_inflate_kernel(const unsigned char* __restrict__ d_in, const StreamDesc* __restrict__ table, unsigned char* __restrict__ d_out,
	int32_t* __restrict__ status, uint64_t* __restrict__ out_bytes, uint64_t* __restrict__ in_bytes, uint32_t* __restrict__ crc)
{
	__shared__ Lds lds;
	const uint64_t s = blockIdx.x;
	const StreamDesc d = table[s];
	const unsigned char* src = d_in + d.in_begin;
	unsigned char* dst = d_out + d.out_begin;
	const Result r = inflate_stream(lds, src, d.in_bytes, (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3), dst, d.out_capacity, (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3));
	if (threadIdx.x == 0) {
		status[s] = r.status;
		out_bytes[s] = r.out_bytes;
		in_bytes[s] = r.in_bytes;
		crc[s] = r.crc;
	}
}

} // namespace

extern "C" int tp_inflate(tp_ctx* ctx, const void* d_in, const uint64_t* h_in_offsets, int64_t n_streams, void* d_out, const uint64_t* h_out_offsets,
	int32_t* d_status, uint64_t* d_out_bytes, uint64_t* d_in_bytes, uint32_t* d_crc)
{
	TP_CHECK_CTX(ctx);
	TP_API_BEGIN
	const char* msg = check(reinterpret_cast<uintptr_t>(d_in), h_in_offsets, n_streams, reinterpret_cast<uintptr_t>(d_out), h_out_offsets, reinterpret_cast<uintptr_t>(d_status),
		reinterpret_cast<uintptr_t>(d_out_bytes), reinterpret_cast<uintptr_t>(d_in_bytes), reinterpret_cast<uintptr_t>(d_crc));
	TP_REQUIRE(ctx, msg == nullptr, msg);
	TP_REQUIRE(ctx, n_streams < ((int64_t)1 << 31), "tp_inflate: a call holds fewer than 2^31 streams");
	std::vector<StreamDesc> table((size_t)n_streams);
	stream_table(h_in_offsets, h_out_offsets, n_streams, table.data());
	// the stream table goes up in one transfer; its block returns to the context's cache behind the kernel
	void* d_table = nullptr;
	int rc = tp_malloc(ctx, (uint64_t)n_streams * sizeof(StreamDesc), &d_table);
	if (rc != TP_OK) return rc;
	rc = tp_memcpy_h2d(ctx, d_table, table.data(), (uint64_t)n_streams * sizeof(StreamDesc));
	if (rc != TP_OK) { (void)tp_free(ctx, d_table); return rc; }
	TP_LAUNCH(ctx, TPK_INFLATE, tp_inflate_kernel, dim3((unsigned)n_streams), dim3(kLanes), 0, static_cast<const unsigned char*>(d_in), static_cast<const StreamDesc*>(d_table),
		static_cast<unsigned char*>(d_out), d_status, d_out_bytes, d_in_bytes, d_crc);
	const hipError_t launched = hipGetLastError();
	(void)tp_free(ctx, d_table);
	if (launched != hipSuccess) return ctx->fail(TP_ERR_HIP, "tp_inflate_kernel", launched);
	return TP_OK;
	TP_API_END(ctx)
}
