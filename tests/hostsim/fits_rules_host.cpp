// Host driver of the FITS unpacker's device-free rules (photometry_amd/csrc/fits_rules.h), built with -fsanitize=address,undefined by
// tests/test_ffi_host.py.  It reads commands from stdin (tokens separated by white space; bit patterns travel in hexadecimal) and
// answers every command with lines on stdout:
//   item N b1 .. bN                        -> N x item_bytes(BITPIX)
//   unpack N, then N x (raw_addr bitpix naxis1 naxis2 row0 col0 rows cols out_addr pitch; addresses in hex)
//                                          -> N x "ok" | "refused MSG"
//   plan N, then N x (raw_addr item naxis1 row0 col0 cols out_addr pitch; addresses in hex)
//                                          -> N x "vec head body4 tail"
//   cvt N x1 .. xN (float64 bits)          -> N x the float32 bits of f64_to_f32_bits, and of the compiler's own cast
//   fold N s1 .. sN (64-bit sums)          -> N x fold32
//   wordsum N, then N x (count word)       -> N x fold32 of the 64-bit sum of `count` copies of `word`, added one by one in uint64
//   datasum N, then N x (raw_addr nbytes sum_addr) -> N x "ok blocks" | "refused MSG"
#include "fits_rules.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace tp_fits;

namespace {

int64_t rd() { long long v; if (!(std::cin >> v)) { std::printf("FAILED: input ended\n"); std::exit(1); } return (int64_t)v; }
uint64_t rd_hex() { std::string s; if (!(std::cin >> s)) { std::printf("FAILED: input ended\n"); std::exit(1); } return std::strtoull(s.c_str(), nullptr, 16); }

} // namespace

int main()
{
	std::string cmd;
	while (std::cin >> cmd) {
		const int64_t n = rd();
		if (cmd == "item") {
			for (int64_t i = 0; i < n; i++) std::printf("%d\n", item_bytes((int32_t)rd()));
		} else if (cmd == "unpack") {
			for (int64_t i = 0; i < n; i++) {
				const uint64_t raw = rd_hex();
				int64_t a[7];
				for (auto& v : a) v = rd();
				const uint64_t out = rd_hex();
				const int64_t pitch = rd();
				const char* msg = unpack_check(raw, (int32_t)a[0], a[1], a[2], a[3], a[4], a[5], a[6], out, pitch);
				if (msg) std::printf("refused %s\n", msg);
				else std::printf("ok\n");
			}
		} else if (cmd == "plan") {
			for (int64_t i = 0; i < n; i++) {
				const uint64_t raw = rd_hex();
				const int item = (int)rd();
				const int64_t naxis1 = rd(), row0 = rd(), col0 = rd(), cols = rd();
				const uint64_t out = rd_hex();
				const int64_t pitch = rd();
				const RowPlan p = row_plan(raw, item, naxis1, row0, col0, cols, out, pitch);
				std::printf("%d %" PRId64 " %" PRId64 " %" PRId64 "\n", p.vec, p.head, p.body4, p.tail);
			}
		} else if (cmd == "cvt") {
			for (int64_t i = 0; i < n; i++) {
				const uint64_t b = rd_hex();
				double d;
				std::memcpy(&d, &b, 8);
				const float f = (float)d;
				uint32_t fb;
				std::memcpy(&fb, &f, 4);
				std::printf("%08x %08x\n", f64_to_f32_bits(b), fb);
			}
		} else if (cmd == "fold") {
			for (int64_t i = 0; i < n; i++) std::printf("%" PRIx64 "\n", fold32(rd_hex()));
		} else if (cmd == "wordsum") {
			for (int64_t i = 0; i < n; i++) {
				const int64_t count = rd();
				const uint64_t word = rd_hex();
				uint64_t s = 0;
				for (int64_t k = 0; k < count; k++) s += word;
				std::printf("%" PRIx64 " %" PRIx64 "\n", s, fold32(s));
			}
		} else if (cmd == "datasum") {
			for (int64_t i = 0; i < n; i++) {
				const uint64_t raw = rd_hex(), nbytes = rd_hex(), sum = rd_hex();
				const char* msg = datasum_check(raw, nbytes, sum);
				if (msg) std::printf("refused %s\n", msg);
				else std::printf("ok %" PRId64 "\n", sum_blocks(nbytes / 16));
			}
		} else {
			std::printf("FAILED: unknown command %s\n", cmd.c_str());
			return 1;
		}
	}
	return 0;
}
