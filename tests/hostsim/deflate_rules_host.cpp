// Host driver of the DEFLATE encoder's device-free rules (photometry_amd/csrc/deflate_rules.h), built with
// -fsanitize=address,undefined by tests/test_deflate_rules_host.py.  It reads commands from stdin (tokens separated by white space)
// and answers every command with lines on stdout:
//   deflate in_file out_file n_streams off_0 .. off_n out_capacity work_bytes null_mask misalign_mask
//       tp_deflate as the library runs it, the rules composed serially -- every chunk, every group, every lane, in the kernel's
//       order of steps -- on the bytes of in_file (read into a buffer of exactly its size).  out_capacity = -1: the sum of the bounds,
//       work_bytes = -1: what tp_deflate_work_bytes asks for; both buffers have exactly that size.  null_mask: 1 d_in, 2 d_out,
//       4 d_chunk_end, 8 d_chunk_crc, 16 d_work, 32 the offsets; misalign_mask: 4 d_chunk_end, 8 d_chunk_crc, 16 d_work.
//       -> "refused MSG" (no out_file), or "ok chunks N total B", N lines "chunk END CRC FORM TOKENS" (behind a dynamic chunk's a
//       line "ll l_0 .. l_285", its literal/length code lengths) and out_file with the B packed bytes; "FAILED ..." when a byte behind the total was written or a chunk's size is not the size its form was chosen by
//   codes n max_bits f_0 .. f_(n-1)   -> "lengths l_0 .. l_(n-1)": build_lengths on the counts
//   combine crc_a crc_b len_b          -> crc_combine
//   bound nbytes                       -> bound_of; "chunk" -> TP_DEFLATE_CHUNK
#include "deflate_rules.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

using namespace tp_deflate_rules;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
std::string rd_str() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return s; }

struct ChunkResult {
	uint32_t bytes, crc, form, tokens;
	std::vector<int> ll;                                       // the literal/length code lengths of a dynamic block
};

// the stage's full words out to the slot, the open word to the front (flush_stage of the kernel)
uint32_t flush_stage(Lds& lds, uint32_t at, uint32_t* slot, uint32_t* word_base)
{
	const uint32_t full = at >> 5;
	for (uint32_t w = 0; w < full; w++) slot[*word_base + w] = lds.stage[w];
	const uint32_t open = lds.stage[full];
	for (uint32_t w = 0; w <= full; w++) lds.stage[w] = 0;
	lds.stage[0] = open;
	*word_base += full;
	return at & 31;
}

// one chunk as its wavefront treats it
ChunkResult encode_chunk(const unsigned char* src, uint32_t n, uint32_t* tokens, uint32_t* slot)
{
	std::unique_ptr<Lds> state(new Lds);
	std::memset(state.get(), 0xA5, sizeof(Lds));               // LDS is stale when a workgroup begins
	Lds& lds = *state;
	const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3);
	// load
	for (int lane = 0; lane < kLanes; lane++) reset(lds, lane, kLanes);
	for (uint32_t w = 0; w < load_words(n, shift); w++) lds.in_words[w] = load_word(src, n, shift, w);
	const unsigned char* in = input_of(lds, shift);
	// checksum
	uint32_t crc = 0;
	for (int lane = 0; lane < kLanes; lane++) crc ^= crc_slice_term(lds.crc_table, in, n, lane);
	// parse
	uint32_t cur = 0, n_tokens = 0;
	for (uint32_t base = 0; base < n; base += kLanes) {
		uint32_t match[kLanes], token[kLanes];
		bool chosen[kLanes];
		uint64_t mask = 0;
		for (int lane = 0; lane < kLanes; lane++) {
			const uint32_t p = base + lane;
			match[lane] = (p < n && p >= cur) ? find_match(in, lds.u.hash, p, n) : 0u;
			if ((match[lane] >> 16) >= (uint32_t)kMinMatch) mask |= (uint64_t)1 << lane;
			chosen[lane] = false;
			token[lane] = 0;
		}
		for (int lane = kLanes - 1; lane >= 0; lane--)          // (any order: an integer maximum)
			if (base + lane < n) hash_insert(in, lds.u.hash, base + lane, n);
		const uint32_t end = base + kLanes < n ? base + kLanes : n;
		while (cur < end) {
			const int from = (int)(cur - base), ml = next_match_lane(mask, from);
			for (int lane = from; lane < ml && base + lane < n; lane++) { chosen[lane] = true; token[lane] = literal_token(in[base + lane]); }
			if (ml == kLanes) { cur = end; break; }
			chosen[ml] = true;
			token[ml] = match_token(match[ml]);
			cur = base + ml + (match[ml] >> 16);
		}
		for (int lane = 0; lane < kLanes; lane++)
			if (chosen[lane]) { tokens[n_tokens++] = token[lane]; count_token(lds, token[lane]); }
	}
	// build
	for (int lane = 0; lane < kLanes; lane++) sort_symbols(lds.freq_ll, kNumLL, lds.u.b.sorted, lane, kLanes);
	build_codes(lds, n);
	// emit
	ChunkResult r{0, crc, lds.form, n_tokens, {}};
	if (lds.form == kFormDynamic) r.ll.assign(lds.len_ll, lds.len_ll + kNumLL);
	if (lds.form == kFormStored) {
		r.bytes = (uint32_t)stored_bytes(n);
		for (uint32_t w = 0; w < (r.bytes + 3) / 4; w++) slot[w] = stored_word(in, n, w);
		return r;
	}
	uint32_t word_base = 0, at = put_header(lds);
	at = flush_stage(lds, at, slot, &word_base);
	for (uint32_t t0 = 0; t0 < n_tokens; t0 += kLanes) {
		uint32_t behind = 0;
		for (int lane = 0; lane < kLanes && t0 + lane < n_tokens; lane++) {
			int nbits = 0;
			const uint64_t bits = token_bits(lds, tokens[t0 + lane], &nbits);
			or_bits(lds.stage, at + behind, bits, nbits);
			behind += (uint32_t)nbits;
		}
		at = flush_stage(lds, at + behind, slot, &word_base);
	}
	at = put_tail(lds, at);
	for (uint32_t w = 0; w < (at + 31) / 32; w++) slot[word_base + w] = lds.stage[w];
	r.bytes = word_base * 4 + at / 8;
	if (r.bytes != lds.coded_bytes) { std::printf("FAILED: a chunk of %u bytes where its form was chosen at %u\n", r.bytes, lds.coded_bytes); std::exit(1); }
	return r;
}

int deflate()
{
	const std::string in_file = rd_str(), out_file = rd_str();
	const int64_t n_streams = rd();
	std::vector<uint64_t> offsets;
	for (int64_t s = 0; s <= (n_streams < 0 ? 0 : n_streams); s++) offsets.push_back((uint64_t)rd());
	const int64_t cap_arg = rd(), work_arg = rd(), null_mask = rd(), misalign = rd();

	std::ifstream f(in_file, std::ios::binary | std::ios::ate);
	const size_t in_bytes = f ? (size_t)f.tellg() : 0;
	std::unique_ptr<unsigned char[]> input(new unsigned char[in_bytes ? in_bytes : 1]);
	if (in_bytes) { f.seekg(0); f.read(reinterpret_cast<char*>(input.get()), (std::streamsize)in_bytes); }

	uint64_t chunks = 0, bound = 0;
	bool rising = n_streams >= 1;
	for (int64_t s = 0; rising && s < n_streams; s++) rising = offsets[s + 1] >= offsets[s];
	if (rising && offsets[n_streams] - offsets[0] < ((uint64_t)1 << 30)) {
		if (offsets[n_streams] > in_bytes) { std::printf("FAILED: the offsets leave the input file\n"); return 1; }
		for (int64_t s = 0; s < n_streams; s++) { chunks += n_chunks_of(offsets[s + 1] - offsets[s]); bound += bound_of(offsets[s + 1] - offsets[s]); }
	}
	const uint64_t capacity = cap_arg < 0 ? bound : (uint64_t)cap_arg, work_bytes = work_arg < 0 ? work_layout(chunks).total : (uint64_t)work_arg;
	constexpr unsigned char kSentinel = 0xC7;
	std::unique_ptr<unsigned char[]> out(new unsigned char[capacity ? capacity : 1]), work(new unsigned char[work_bytes + 16]);
	std::unique_ptr<uint64_t[]> ends(new uint64_t[chunks + 2]);
	std::unique_ptr<uint32_t[]> crcs(new uint32_t[chunks + 2]);
	std::memset(out.get(), kSentinel, capacity ? capacity : 1);
	const uint64_t in_addr = (null_mask & 1) ? 0 : reinterpret_cast<uintptr_t>(input.get());
	const uint64_t out_addr = (null_mask & 2) ? 0 : reinterpret_cast<uintptr_t>(out.get());
	const uint64_t end_addr = (null_mask & 4) ? 0 : reinterpret_cast<uintptr_t>(ends.get()) + ((misalign & 4) ? 4 : 0);
	const uint64_t crc_addr = (null_mask & 8) ? 0 : reinterpret_cast<uintptr_t>(crcs.get()) + ((misalign & 8) ? 2 : 0);
	const uint64_t work_addr = (null_mask & 16) ? 0 : reinterpret_cast<uintptr_t>(work.get()) + ((misalign & 16) ? 8 : 0);
	uint64_t n_chunks = 0;
	const char* msg = check(in_addr, (null_mask & 32) ? nullptr : offsets.data(), n_streams, out_addr, capacity, end_addr, crc_addr, work_addr, work_bytes, &n_chunks);
	if (msg) { std::printf("refused %s\n", msg); return 0; }

	std::vector<ChunkDesc> table((size_t)n_chunks);
	chunk_table(offsets.data(), n_streams, table.data());
	const WorkLayout lay = work_layout(n_chunks);
	std::vector<ChunkResult> results;
	uint32_t* sizes = reinterpret_cast<uint32_t*>(work.get() + lay.sizes);
	for (uint64_t c = 0; c < n_chunks; c++) {
		results.push_back(encode_chunk(input.get() + table[c].offset, table[c].nbytes, reinterpret_cast<uint32_t*>(work.get() + lay.tokens) + c * (uint64_t)kChunk,
			reinterpret_cast<uint32_t*>(work.get() + lay.slots) + c * (uint64_t)(kSlotBytes / 4)));
		sizes[c] = results.back().bytes;
		crcs[c] = results.back().crc;
		if (results.back().bytes > table[c].nbytes + (uint32_t)kChunkGrowth) { std::printf("FAILED: chunk %" PRIu64 " grew past the bound\n", c); return 1; }
	}
	uint64_t run = 0;
	for (uint64_t c = 0; c < n_chunks; c++) { run += sizes[c]; ends[c] = run; }
	for (uint64_t c = 0; c < n_chunks; c++)
		std::memcpy(out.get() + (ends[c] - sizes[c]), work.get() + lay.slots + c * (uint64_t)kSlotBytes, sizes[c]);
	for (uint64_t k = run; k < capacity; k++)
		if (out[k] != kSentinel) { std::printf("FAILED: byte %" PRIu64 " behind the total was written\n", k); return 1; }
	std::ofstream of(out_file, std::ios::binary);
	of.write(reinterpret_cast<const char*>(out.get()), (std::streamsize)run);
	std::printf("ok chunks %" PRIu64 " total %" PRIu64 "\n", n_chunks, run);
	for (uint64_t c = 0; c < n_chunks; c++) {
		std::printf("chunk %" PRIu64 " %u %u %u\n", ends[c], results[c].crc, results[c].form, results[c].tokens);
		if (!results[c].ll.empty()) {
			std::printf("ll");
			for (int l : results[c].ll) std::printf(" %d", l);
			std::printf("\n");
		}
	}
	return 0;
}

int codes()
{
	const int n = (int)rd(), max_bits = (int)rd();
	if (n < 1 || n > 288 || max_bits < 1 || max_bits > 15) { std::printf("FAILED: codes arguments\n"); return 1; }
	std::vector<uint32_t> freq(n), a(n), count(16);
	std::vector<uint16_t> sorted(n);
	std::vector<uint8_t> len(n);
	for (auto& v : freq) v = (uint32_t)rd();
	for (int lane = 0; lane < kLanes; lane++) sort_symbols(freq.data(), n, sorted.data(), lane, kLanes);
	build_lengths(freq.data(), n, max_bits, len.data(), sorted.data(), a.data(), count.data());
	std::printf("lengths");
	for (int s = 0; s < n; s++) std::printf(" %d", (int)len[s]);
	std::printf("\n");
	return 0;
}

} // namespace

int main()
{
	std::string cmd;
	while (std::cin >> cmd) {
		if (cmd == "deflate") {
			if (deflate()) return 1;
		} else if (cmd == "codes") {
			if (codes()) return 1;
		} else if (cmd == "combine") {
			const uint32_t a = (uint32_t)rd(), b = (uint32_t)rd();
			const uint64_t len = (uint64_t)rd();
			std::printf("%u\n", crc_combine(a, b, len));
		} else if (cmd == "bound") {
			std::printf("%" PRIu64 "\n", bound_of((uint64_t)rd()));
		} else if (cmd == "chunk") {
			std::printf("%d\n", kChunk);
		} else {
			std::printf("FAILED: unknown command %s\n", cmd.c_str());
			return 1;
		}
		std::fflush(stdout);
	}
	return 0;
}
