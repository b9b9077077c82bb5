// Host driver of the light-curve table packer's rules (photometry_amd/csrc/lctable_rules.h): composes them serially -- every target, every
// tile, every lane, every piece -- into the bytes tp_lc_table_pack and tp_lc_place write, with every buffer of exactly the size a call
// may touch, so that AddressSanitizer and UBSan see any index that leaves one.  Commands on stdin, one per line:
//   pack IN OUT n_targets T n_rows has_rows  n_time s  n_timecorr s  n_cadenceno s  n_pixel_quality s  n_lc plane_stride target_stride
//        n_quality s  n_pos_corr s  capacity null_mask misalign_mask  offset[n_targets]
//     IN holds the arrays in this order (float64 / int32 as in the source description, n_quality or n_pos_corr -1: a null pointer),
//     then n_rows int32 kept rows when has_rows.  OUT receives the `capacity` bytes of the output buffer, pre-filled with 0xA5, then
//     n_targets uint64 sums.  Prints `ok` or `refused MESSAGE` (OUT is then not written).
//     null_mask: 1 time, 2 timecorr, 4 cadenceno, 8 pixel_quality, 16 lc, 32 out, 64 sums, 128 offsets, 256 the description itself.
//     misalign_mask: 32 out, 64 sums, 512 rows.
//   place IN OUT src_capacity dst_capacity n_segments null_mask misalign_mask  (src_offset dst_offset length)[n_segments]
//     IN holds the src_capacity source bytes; OUT receives the dst_capacity bytes, pre-filled with 0xA5.
//     null_mask: 1 src, 2 dst, 4 the offset arrays.  misalign_mask: 1 src, 2 dst.
//   maxrows -- prints kMaxRows and whether kMaxRows rows of all-ones words fit in 64 bits while kMaxRows + 1 rows do not.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "lctable_rules.h"

using namespace tp_lctable;

namespace {

// an allocation of exactly `bytes` bytes (at least one, so that the pointer is not null), 16-byte aligned
struct Exact {
	void* p = nullptr;
	explicit Exact(size_t bytes) { if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) abort(); }
	~Exact() { free(p); }
	Exact(const Exact&) = delete;
	Exact& operator=(const Exact&) = delete;
};

bool read_exact(FILE* fh, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, fh) == bytes; }

void pack(const Src& src, const int32_t* rows, int64_t n_rows, int64_t T, int64_t n_targets, unsigned char* out, const uint64_t* offsets, uint64_t* sums)
{
	for (int64_t i = 0; i < n_targets; i++) sums[i] = 0;
	const int64_t padded = padded_rows(n_rows);
	const int64_t per_target = blocks_per_target(n_rows);
	for (int64_t block = 0; block < per_target * n_targets; block++) {
		const int64_t target = block / per_target;
		for (int wave = 0; wave < kWaves; wave++) {
			const int64_t tile = (block % per_target) * kWaves + wave;
			std::vector<uint32_t> tl(kLdsTileWords, 0xDEADBEEFu);
			uint64_t sum = 0;
			for (int lane = 0; lane < 64; lane++) {
				const int64_t r = tile * kTileRows + lane;
				if (r >= padded) continue;
				uint32_t w[kRowWords] = {};
				if (r < n_rows) {
					const RowValues v = load_row(src, target, row_cadence(rows, r, T));
					row_words(v, w);
					sum += row_sum(v);
				}
				for (int p = 0; p < kRowPieces; p++)
					for (int j = 0; j < 4; j++) tl.at(lds_index(lane, 4 * p) + j) = w[4 * p + j];
			}
			for (int step = 0; step < kPieceSteps; step++)
				for (int lane = 0; lane < 64; lane++) {
					const Piece p = piece_of(lane, step);
					if (tile * kTileRows + p.row < padded) {
						(void)tl.at(lds_index(p.row, p.word) + 3);
						memcpy(out + offsets[target] + tile * kTileBytes + p.byte, &tl[lds_index(p.row, p.word)], 16);
					}
				}
			if (tile * kTileRows < n_rows) sums[target] += sum;
		}
	}
	for (int64_t i = 0; i < n_targets; i++) sums[i] = fold32(sums[i]);
}

int do_pack(std::istringstream& in)
{
	std::string in_path, out_path;
	int64_t n_targets, T, n_rows, has_rows, n[7], stride[7], target_stride, capacity, null_mask, misalign_mask;
	in >> in_path >> out_path >> n_targets >> T >> n_rows >> has_rows;
	for (int k = 0; k < 7; k++) {
		in >> n[k] >> stride[k];
		if (k == 4) in >> target_stride;
	}
	in >> capacity >> null_mask >> misalign_mask;
	std::vector<uint64_t> offsets;
	offsets.reserve(1);                                 // (a pointer that is not null for a call without targets)
	for (int64_t i = 0; i < n_targets; i++) { uint64_t o; in >> o; offsets.push_back(o); }
	if (!in) { printf("FAILED to parse\n"); return 1; }
	const int item[7] = {8, 8, 4, 4, 8, 4, 8};
	std::vector<Exact*> held;
	void* ptr[7];
	FILE* fh = fopen(in_path.c_str(), "rb");
	if (!fh) { printf("FAILED to open\n"); return 1; }
	for (int k = 0; k < 7; k++) {
		if (n[k] < 0) { ptr[k] = nullptr; continue; }
		held.push_back(new Exact((size_t)n[k] * item[k]));
		ptr[k] = held.back()->p;
		if (!read_exact(fh, ptr[k], (size_t)n[k] * item[k])) { printf("FAILED to read\n"); return 1; }
	}
	const int64_t n_list = has_rows && n_rows > 0 ? n_rows : 0;
	Exact rows_block((size_t)n_list * 4);
	if (!read_exact(fh, rows_block.p, (size_t)n_list * 4)) { printf("FAILED to read\n"); return 1; }
	fclose(fh);
	const int32_t* rows = has_rows ? static_cast<const int32_t*>(rows_block.p) : nullptr;
	Src src{};
	src.time = (null_mask & 1) ? nullptr : static_cast<const uint64_t*>(ptr[0]); src.time_stride = stride[0];
	src.timecorr = (null_mask & 2) ? nullptr : static_cast<const uint64_t*>(ptr[1]); src.timecorr_stride = stride[1];
	src.cadenceno = (null_mask & 4) ? nullptr : static_cast<const int32_t*>(ptr[2]); src.cadenceno_stride = stride[2];
	src.pixel_quality = (null_mask & 8) ? nullptr : static_cast<const int32_t*>(ptr[3]); src.pixel_quality_stride = stride[3];
	src.lc = (null_mask & 16) ? nullptr : static_cast<const uint64_t*>(ptr[4]); src.lc_plane_stride = stride[4]; src.lc_target_stride = target_stride;
	src.quality = static_cast<const int32_t*>(ptr[5]); src.quality_stride = stride[5];
	src.pos_corr = static_cast<const uint64_t*>(ptr[6]); src.pos_corr_stride = stride[6];
	Exact out_block((size_t)capacity + 16), sum_block((size_t)(n_targets > 0 ? n_targets : 0) * 8 + 8);
	unsigned char* out = static_cast<unsigned char*>(out_block.p);
	memset(out, 0xA5, (size_t)capacity);
	uint64_t* sums = static_cast<uint64_t*>(sum_block.p);
	const uint64_t out_addr = (null_mask & 32) ? 0 : reinterpret_cast<uintptr_t>(out) + ((misalign_mask & 32) ? 8 : 0);
	const uint64_t sum_addr = (null_mask & 64) ? 0 : reinterpret_cast<uintptr_t>(sums) + ((misalign_mask & 64) ? 4 : 0);
	const uint64_t rows_addr = reinterpret_cast<uintptr_t>(rows) + ((misalign_mask & 512) ? 2 : 0);
	const char* msg = pack_check((null_mask & 256) ? nullptr : &src, rows_addr, n_rows, T, n_targets, out_addr, (null_mask & 128) ? nullptr : offsets.data(), (uint64_t)capacity,
		sum_addr);
	int rc = 0;
	if (msg != nullptr) printf("refused %s\n", msg);
	else {
		// the buffers of the run itself: exactly `capacity` and n_targets * 8 bytes
		Exact exact_out((size_t)capacity), exact_sums((size_t)n_targets * 8);
		memset(exact_out.p, 0xA5, (size_t)capacity);
		pack(src, rows, n_rows, T, n_targets, static_cast<unsigned char*>(exact_out.p), offsets.data(), static_cast<uint64_t*>(exact_sums.p));
		FILE* oh = fopen(out_path.c_str(), "wb");
		if (!oh || fwrite(exact_out.p, 1, (size_t)capacity, oh) != (size_t)capacity || fwrite(exact_sums.p, 8, (size_t)n_targets, oh) != (size_t)n_targets) { printf("FAILED to write\n"); rc = 1; }
		else printf("ok\n");
		if (oh) fclose(oh);
	}
	for (Exact* e : held) delete e;
	return rc;
}

int do_place(std::istringstream& in)
{
	std::string in_path, out_path;
	int64_t src_capacity, dst_capacity, n_segments, null_mask, misalign_mask;
	in >> in_path >> out_path >> src_capacity >> dst_capacity >> n_segments >> null_mask >> misalign_mask;
	std::vector<uint64_t> so, dof, len;
	so.reserve(1); dof.reserve(1); len.reserve(1);      // (pointers that are not null for a call without segments)
	for (int64_t k = 0; k < n_segments; k++) { uint64_t a, b, c; in >> a >> b >> c; so.push_back(a); dof.push_back(b); len.push_back(c); }
	if (!in) { printf("FAILED to parse\n"); return 1; }
	Exact src((size_t)src_capacity), dst((size_t)dst_capacity);
	FILE* fh = fopen(in_path.c_str(), "rb");
	if (!fh || !read_exact(fh, src.p, (size_t)src_capacity)) { printf("FAILED to read\n"); return 1; }
	fclose(fh);
	memset(dst.p, 0xA5, (size_t)dst_capacity);
	const uint64_t src_addr = (null_mask & 1) ? 0 : reinterpret_cast<uintptr_t>(src.p) + ((misalign_mask & 1) ? 8 : 0);
	const uint64_t dst_addr = (null_mask & 2) ? 0 : reinterpret_cast<uintptr_t>(dst.p) + ((misalign_mask & 2) ? 8 : 0);
	const bool no_arrays = (null_mask & 4) != 0;
	const char* msg = place_check(src_addr, (uint64_t)src_capacity, no_arrays ? nullptr : so.data(), no_arrays ? nullptr : dof.data(), no_arrays ? nullptr : len.data(), n_segments,
		dst_addr, (uint64_t)dst_capacity);
	if (msg != nullptr) { printf("refused %s\n", msg); return 0; }
	std::vector<uint64_t> first(n_segments + 1, 0);
	for (int64_t k = 0; k < n_segments; k++) first[k + 1] = first[k] + len[k] / 16;
	for (uint64_t g = 0; g < first[n_segments]; g++) {
		const int64_t k = segment_of(first.data(), n_segments, g);
		const uint64_t within = 16 * (g - first.at(k));
		memcpy(static_cast<unsigned char*>(dst.p) + dof.at(k) + within, static_cast<const unsigned char*>(src.p) + so.at(k) + within, 16);
	}
	FILE* oh = fopen(out_path.c_str(), "wb");
	if (!oh || fwrite(dst.p, 1, (size_t)dst_capacity, oh) != (size_t)dst_capacity) { printf("FAILED to write\n"); return 1; }
	fclose(oh);
	printf("ok\n");
	return 0;
}

} // namespace

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		int rc = 0;
		if (cmd == "pack") rc = do_pack(in);
		else if (cmd == "place") rc = do_place(in);
		else if (cmd == "maxrows") {
			const unsigned __int128 worst = (unsigned __int128)kRowWords * 0xFFFFFFFFull;
			const unsigned __int128 limit = (unsigned __int128)1 << 64;
			printf("%lld %d %d\n", (long long)kMaxRows, (int)(worst * (unsigned __int128)kMaxRows < limit), (int)(worst * (unsigned __int128)(kMaxRows + 1) < limit));
		} else if (!cmd.empty()) { printf("FAILED: unknown command\n"); rc = 1; }
		if (rc != 0) return rc;
	}
	return 0;
}
