// Host driver of the DEFLATE decoder's device-free rules (photometry_amd/csrc/inflate_rules.h), built with
// -fsanitize=address,undefined by tests/inflate_common.py.  It reads commands from stdin (tokens separated by white space) and
// answers every command with lines on stdout:
//   inflate in_file out_file n_streams in_0 .. in_n out_0 .. out_n null_mask misalign_mask
//       tp_inflate as the library runs it: inflate_stream of the rules on every stream, the pieces the lanes share run lane after
//       lane.  Stream s is the bytes [in_s, in_(s+1)) of in_file and has a slot of out_(s+1) - out_s bytes.  Every stream's input and
//       slot are buffers of their own, of exactly their size behind the address's low two bits the call would give them (the bytes in
//       front are poisoned), the slot filled with a sentinel.  null_mask: 1 d_in, 2 d_out, 4 d_status, 8 d_out_bytes, 16 d_in_bytes,
//       32 d_crc, 64 the input offsets, 128 the output offsets; misalign_mask: 4 d_status, 8 d_out_bytes, 16 d_in_bytes, 32 d_crc.
//       -> "refused MSG" (no out_file), or "ok streams N", N lines "stream STATUS OUT_BYTES IN_BYTES CRC" and out_file with the bytes
//       the streams produced, back to back; "FAILED ..." when a slot byte behind the bytes produced was written
//   bases -> the smallest length of the symbols 257 .. 285 and the smallest distance of the symbols 0 .. 29
//   lds   -> sizeof(Lds)
#include "inflate_rules.h"
#include <sanitizer/asan_interface.h>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

using namespace tp_inflate_rules;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
std::string rd_str() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return s; }

constexpr unsigned char kSentinel = 0xC7;

// n bytes whose first one has the address's low two bits `shift`, nothing addressable around them
struct Exact {
	std::unique_ptr<unsigned char[]> block;
	unsigned char* at;
	uint32_t shift;
	uint64_t bytes;
	Exact(uint64_t n, uint32_t s) : block(new unsigned char[n + s + 1]), at(block.get() + s), shift(s), bytes(n)
	{
		// (operator new gives 16-byte alignment; one byte more than asked so that an empty stream has an address.  The byte behind is
		// poisoned exactly; of the up to three bytes in front the sanitizer poisons what its 8-byte shadow granules can express)
		ASAN_POISON_MEMORY_REGION(block.get(), s);
		ASAN_POISON_MEMORY_REGION(at + n, 1);
	}
	~Exact() { ASAN_UNPOISON_MEMORY_REGION(block.get(), bytes + shift + 1); }
};

int inflate()
{
	const std::string in_file = rd_str(), out_file = rd_str();
	const int64_t n_streams = rd();
	const int64_t n_off = n_streams < 0 ? 0 : n_streams;
	std::vector<uint64_t> in_off, out_off;
	for (int64_t s = 0; s <= n_off; s++) in_off.push_back((uint64_t)rd());
	for (int64_t s = 0; s <= n_off; s++) out_off.push_back((uint64_t)rd());
	const int64_t null_mask = rd(), misalign = rd();

	std::ifstream f(in_file, std::ios::binary | std::ios::ate);
	const size_t in_bytes = f ? (size_t)f.tellg() : 0;
	std::vector<unsigned char> input(in_bytes);
	if (in_bytes) { f.seekg(0); f.read(reinterpret_cast<char*>(input.data()), (std::streamsize)in_bytes); }

	std::unique_ptr<int32_t[]> status(new int32_t[n_off + 2]);
	std::unique_ptr<uint64_t[]> produced(new uint64_t[n_off + 2]), consumed(new uint64_t[n_off + 2]);
	std::unique_ptr<uint32_t[]> crcs(new uint32_t[n_off + 2]);
	const uint64_t base_in = 0x1000, base_out = 0x2000;            // the call's d_in and d_out as far as the refusals and the shifts go
	const uint64_t in_addr = (null_mask & 1) ? 0 : base_in, out_addr = (null_mask & 2) ? 0 : base_out;
	const uint64_t status_addr = (null_mask & 4) ? 0 : reinterpret_cast<uintptr_t>(status.get()) + ((misalign & 4) ? 2 : 0);
	const uint64_t produced_addr = (null_mask & 8) ? 0 : reinterpret_cast<uintptr_t>(produced.get()) + ((misalign & 8) ? 4 : 0);
	const uint64_t consumed_addr = (null_mask & 16) ? 0 : reinterpret_cast<uintptr_t>(consumed.get()) + ((misalign & 16) ? 4 : 0);
	const uint64_t crc_addr = (null_mask & 32) ? 0 : reinterpret_cast<uintptr_t>(crcs.get()) + ((misalign & 32) ? 2 : 0);
	const char* msg = check(in_addr, (null_mask & 64) ? nullptr : in_off.data(), n_streams, out_addr, (null_mask & 128) ? nullptr : out_off.data(), status_addr,
		produced_addr, consumed_addr, crc_addr);
	if (msg) { std::printf("refused %s\n", msg); return 0; }
	if (in_off[n_streams] > in_bytes) { std::printf("FAILED: the offsets leave the input file\n"); return 1; }

	std::vector<StreamDesc> table((size_t)n_streams);
	stream_table(in_off.data(), out_off.data(), n_streams, table.data());
	std::ofstream of(out_file, std::ios::binary);
	for (int64_t s = 0; s < n_streams; s++) {
		const StreamDesc d = table[(size_t)s];
		Exact src(d.in_bytes, (uint32_t)((base_in + d.in_begin) & 3)), dst(d.out_capacity, (uint32_t)((base_out + d.out_begin) & 3));
		if (d.in_bytes) std::memcpy(src.at, input.data() + d.in_begin, d.in_bytes);
		std::memset(dst.at, kSentinel, d.out_capacity);
		std::unique_ptr<Lds> state(new Lds);
		std::memset(state.get(), 0xA5, sizeof(Lds));               // LDS is stale when a workgroup begins
		const Result r = inflate_stream(*state, src.at, d.in_bytes, src.shift, dst.at, d.out_capacity, dst.shift);
		if (r.out_bytes > d.out_capacity) { std::printf("FAILED: stream %" PRId64 " counts more bytes than its slot holds\n", s); return 1; }
		for (uint64_t k = r.out_bytes; k < d.out_capacity; k++)
			if (dst.at[k] != kSentinel) { std::printf("FAILED: stream %" PRId64 ": byte %" PRIu64 " behind the bytes produced was written\n", s, k); return 1; }
		status[s] = r.status; produced[s] = r.out_bytes; consumed[s] = r.in_bytes; crcs[s] = r.crc;
		of.write(reinterpret_cast<const char*>(dst.at), (std::streamsize)r.out_bytes);
	}
	std::printf("ok streams %" PRId64 "\n", n_streams);
	for (int64_t s = 0; s < n_streams; s++) std::printf("stream %d %" PRIu64 " %" PRIu64 " %u\n", status[s], produced[s], consumed[s], crcs[s]);
	return 0;
}

} // namespace

int main()
{
	std::string cmd;
	while (std::cin >> cmd) {
		if (cmd == "inflate") {
			if (inflate()) return 1;
		} else if (cmd == "bases") {
			for (int s = 257; s <= 285; s++) std::printf("%u ", length_base(s));
			std::printf("\n");
			for (int s = 0; s < 30; s++) std::printf("%u ", distance_base(s));
			std::printf("\n");
		} else if (cmd == "lds") {
			std::printf("%zu\n", sizeof(Lds));
		} else {
			std::printf("FAILED: unknown command %s\n", cmd.c_str());
			return 1;
		}
		std::fflush(stdout);
	}
	return 0;
}
