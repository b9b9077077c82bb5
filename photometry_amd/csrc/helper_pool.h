// helper_pool.h -- the frames engine's helper threads and the fork-join that runs the parts of a job on them (host code only, no HIP:
// tests/hostsim/helper_pool_tsan.cpp compiles it under ThreadSanitizer).
#pragma once
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

// A few helper threads of the engine, started once: the catalogue selection of a large group is cut into runs of stamps and the
// runs are selected side by side (threads started per group cost more than they saved: 2.3 ms against 0.75 for 2 500 stamps).
struct HelperPool {
	std::mutex m;
	std::condition_variable cv;
	std::deque<std::function<void()>> tasks;
	std::vector<std::thread> threads;
	bool stop = false;
	void start(int n) {
		for (int i = 0; i < n; ++i) {
			try {
				threads.emplace_back([this] {
					for (;;) {
						std::function<void()> f;
						{
							std::unique_lock<std::mutex> lk(m);
							cv.wait(lk, [this] { return stop || !tasks.empty(); });
							if (tasks.empty()) return;      // (stop, and nothing left to do)
							f = std::move(tasks.front());
							tasks.pop_front();
						}
						f();
					}
				});
			} catch (...) { break; }                   // fewer helpers, or none: the callers run what nobody takes
		}
	}
	void post(std::function<void()> f) { { std::lock_guard<std::mutex> lk(m); tasks.push_back(std::move(f)); } cv.notify_one(); }
	// a posted task that no helper has taken yet, for the poster to run itself rather than wait
	bool take(std::function<void()>& f) {
		std::lock_guard<std::mutex> lk(m);
		if (tasks.empty()) return false;
		f = std::move(tasks.front());
		tasks.pop_front();
		return true;
	}
	// part(0) .. part(K - 1), returning once every one has finished: part 0 on the calling thread, the others posted to the helpers
	// (what no helper has taken when the caller is through with its own part, or what could not be posted, the caller does itself).
	// An exception of part 0 is rethrown after the join; false if a posted part threw.
	template <class Part>
	bool fork_join(int K, const Part& part) {
		struct Join { std::mutex m; std::condition_variable cv; int pending = 0; bool failed = false; };
		// Invariant: a task calls `part` (the caller's frame) only while it counts in `pending`; after that it touches nothing but its
		// own shared_ptr to the join state.
		const auto st = std::make_shared<Join>();
		st->pending = K - 1;
		auto task = [st, &part](int k) {
			return [st, &part, k] {
				bool ok = true;
				try { part(k); } catch (...) { ok = false; }
				{ std::lock_guard<std::mutex> lk(st->m); st->failed = st->failed || !ok; st->pending -= 1; }
				st->cv.notify_one();
			};
		};
		int posted = 1;
		try { for (; posted < K; ++posted) post(task(posted)); } catch (...) {}   // (out of memory: the rest runs below)
		std::exception_ptr own;
		try { part(0); } catch (...) { own = std::current_exception(); }
		for (int k = posted; k < K; ++k) task(k)();
		std::function<void()> f;                   // (tasks of other callers may be among them: any is as good to do)
		while (take(f)) f();
		{
			std::unique_lock<std::mutex> lk(st->m);
			st->cv.wait(lk, [&] { return st->pending == 0; });
		}
		if (own) std::rethrow_exception(own);
		return !st->failed;
	}
	~HelperPool() {
		{ std::lock_guard<std::mutex> lk(m); stop = true; }
		cv.notify_all();
		for (auto& t : threads) if (t.joinable()) t.join();
	}
};
