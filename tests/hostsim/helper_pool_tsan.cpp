// Host driver of HelperPool::fork_join (photometry_amd/csrc/helper_pool.h), built with -fsanitize=thread by tests/test_helper_pool.py.
// argv[1] picks the case; the driver prints one line "ok ..." and exits 0, or names what went wrong and exits 1.
//   repeat       -- four callers (the engine's workers) and three helpers, many fork-joins each: every caller returns and overwrites the
//                   stack its parts used at once, so a helper that touched the caller's frame or the join state late is a race
//   own_throws   -- part 0 throws while the posted parts are still running: the call waits for them, then rethrows
//   helper_throws -- a posted part throws: the call returns false once every part has finished
#include "helper_pool.h"
#include <chrono>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

namespace {

constexpr int K = 4;

bool fail(const char* what) { std::printf("FAILED: %s\n", what); return false; }

// one fork-join whose state lives in this frame only
__attribute__((noinline)) bool join_once(HelperPool& pool, int rep) {
	int ran[K] = {0, 0, 0, 0};
	volatile long sink[K] = {0, 0, 0, 0};
	const bool ok = pool.fork_join(K, [&](int k) {
		long acc = 0;
		for (int i = 0; i < 50 * (k + 1) + rep % 7; ++i) acc += i ^ k;
		sink[k] = acc;
		ran[k] += 1;
	});
	if (!ok) return fail("fork_join reported a failed part");
	for (int k = 0; k < K; ++k) if (ran[k] != 1) return fail("a part did not run exactly once");
	return true;
}

// reuses the stack that join_once's frame occupied
__attribute__((noinline)) void scribble() {
	volatile char buf[4096];
	for (size_t i = 0; i < sizeof buf; ++i) buf[i] = (char)i;
}

bool repeat() {
	HelperPool pool;
	pool.start(3);
	constexpr int kCallers = 4, kReps = 2000;
	bool ok[kCallers];
	std::vector<std::thread> callers;
	for (int c = 0; c < kCallers; ++c)
		callers.emplace_back([&pool, &ok, c] {
			ok[c] = true;
			for (int r = 0; r < kReps && ok[c]; ++r) { ok[c] = join_once(pool, r); scribble(); }
		});
	for (auto& t : callers) t.join();
	for (int c = 0; c < kCallers; ++c) if (!ok[c]) return false;
	std::printf("ok repeat %d fork-joins\n", kCallers * kReps);
	return true;
}

bool own_throws() {
	HelperPool pool;
	pool.start(3);
	int ran[K] = {0, 0, 0, 0};
	std::string caught;
	try {
		(void)pool.fork_join(K, [&](int k) {
			if (k == 0) { ran[0] += 1; throw std::runtime_error("own part"); }
			std::this_thread::sleep_for(std::chrono::milliseconds(20));   // (still running when part 0 throws)
			ran[k] += 1;
		});
	} catch (const std::runtime_error& e) { caught = e.what(); }
	if (caught != "own part") return fail("the exception of part 0 did not reach the caller");
	for (int k = 0; k < K; ++k) if (ran[k] != 1) return fail("a part did not run exactly once");
	std::printf("ok own_throws %s\n", caught.c_str());
	return true;
}

bool helper_throws() {
	HelperPool pool;
	pool.start(3);
	int ran[K] = {0, 0, 0, 0};
	const bool ok = pool.fork_join(K, [&](int k) {
		if (k == 0) std::this_thread::sleep_for(std::chrono::milliseconds(20));   // (the helpers take their parts first)
		ran[k] += 1;
		if (k == 2) throw std::runtime_error("helper part");
	});
	if (ok) return fail("a part that threw on a helper was not reported");
	for (int k = 0; k < K; ++k) if (ran[k] != 1) return fail("a part did not run exactly once");
	std::printf("ok helper_throws\n");
	return true;
}

} // namespace

int main(int argc, char** argv) {
	const char* c = argc > 1 ? argv[1] : "";
	bool ok;
	if (!std::strcmp(c, "repeat")) ok = repeat();
	else if (!std::strcmp(c, "own_throws")) ok = own_throws();
	else if (!std::strcmp(c, "helper_throws")) ok = helper_throws();
	else { std::printf("unknown case '%s'\n", c); return 2; }
	return ok ? 0 : 1;
}
